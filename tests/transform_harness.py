"""What the tests of msplat_transform_cloud share that talks to the library: msplat_sh_rotation through ctypes, the rule's rows of a
context's download with the library's own D, and the state of a context that was uploaded those rows.  torch is imported inside the
functions that need it.  pytest rewrites `assert` in test modules only, so every assertion here carries its values in its message."""
import ctypes as C

import numpy as np

from splatapult_amd import _capi
from tests import compact_harness as ch
from tests import transform_rule as tr
from tests.gpu_harness import make_renderer

_P = C.POINTER(C.c_float)


def sh_rotation(M, scale=True):
    """(return code, {1: (3, 3), 2: (5, 5), 3: (7, 7)} float32 -- filled with NaN before the call --, scale or None)"""
    m = np.ascontiguousarray(np.asarray(M, np.float32).reshape(16))
    D = {b: np.full((nb, nb), np.nan, np.float32) for b, (_, nb) in tr.BANDS.items()}
    s = C.c_float(np.nan)
    rc = _capi.lib().msplat_sh_rotation(m.ctypes.data_as(_P), D[1].ctypes.data_as(_P), D[2].ctypes.data_as(_P), D[3].ctypes.data_as(_P),
                                        C.byref(s) if scale else None)
    return rc, D, (float(s.value) if scale else None)


def library_D(M):
    rc, D, _ = sh_rotation(M)
    assert rc == _capi.OK, "msplat_sh_rotation: %d" % rc
    return D


def rule_rows(rows, M, select=None, keep_sh=False):
    """the rule of the header on downloaded rows, D being what the library returns for M"""
    return tr.transform_rows(rows, M, None if keep_sh else library_D(M), select)


def uploaded_state(rows, view, mask=None, crop=None, **kw):
    """the reference: the state of a context that was uploaded `rows` (and set the mask / crop)"""
    s = make_renderer(np.ascontiguousarray(rows), **kw)
    if mask is not None:
        s.SetVisibility(mask)
    if crop is not None:
        s.SetCrop(*crop)
    st = ch.context_state(s, view, rows.shape[1] == 61)
    st["visibility"] = s.visibility()
    s.close()
    return st


def assert_same_context_again(got, ref, what):
    """assert_same_context for a context that has sorted before: whether a Sort's first pass walks the listed live boxes only
    depends on the sort_count of an EARLIER frame of the context (the same keys and order either way), so that flag is left out"""
    ch.assert_same_context(dict(got, boxes=got["boxes"][:2]), dict(ref, boxes=ref["boxes"][:2]), what)
