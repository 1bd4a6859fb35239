"""CPU tests of msplat_compact_cloud: the entry point exists in the header, the library and the binding and
refuses a NULL context without a device, and the fixtures of tests/test_gpu_compact.py are what they claim -- every mask case keeps
the count its name says, the sizes sit on the edges of a cull box and of a scan chunk, and the index map is a bijection from the
kept splats onto 0..K-1 in ascending order."""
import ctypes as C
import os

import numpy as np

from splatapult_amd import SplatRenderer, _capi
from tests import compact_rule as cr
from tests import visibility_rule as vr
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")


def test_the_header_declares_the_call_the_library_exports_it_and_a_null_context_is_refused():
    header = open(HEADER).read()
    assert "int msplat_compact_cloud(msplat_ctx* ctx, uint32_t* d_index_map, uint64_t* n_kept_out);" in header
    assert hasattr(C.CDLL(_capi.LIB_PATH), "msplat_compact_cloud"), "libmsplat.so does not export msplat_compact_cloud"
    assert "msplat_compact_cloud" in {n for n, _, _ in _capi.SYMBOLS}, "no ctypes prototype for msplat_compact_cloud"
    assert callable(getattr(SplatRenderer, "CompactCloud", None)), "SplatRenderer has no CompactCloud"
    L = _capi.lib()
    k = C.c_uint64(77)
    assert L.msplat_compact_cloud(None, None, C.byref(k)) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in L.msplat_last_error(None).decode()
    assert k.value == 77                                         # (nothing was written)
    assert L.msplat_compact_cloud(None, None, None) == _capi.ERR_INVALID_ARG


def test_the_header_still_has_at_most_300_lines():
    assert len(open(HEADER).read().splitlines()) <= 300


def test_every_mask_case_keeps_what_its_name_says():
    for n in cr.SIZES:
        cases = cr.mask_cases(n)
        assert set(vr.mask_cases(n)) < set(cases) and {"first_only", "last_only"} <= set(cases)
        assert ("one_chunk_hidden" in cases) == (n >= 2 * cr.CHUNK)
        for name, mask in cases.items():
            assert mask.shape == (n,) and mask.dtype in (np.bool_, np.uint8), (n, name)
            keep = cr.keep_of(mask)
            if name in cr.KEPT_BY_NAME:
                assert keep.sum() == cr.KEPT_BY_NAME[name](n), (n, name, keep.sum())
            else:
                assert name in ("random_30", "bytes_2_255") and 0 < keep.sum() < n, (n, name)
        assert cases["first_only"][0] and cases["last_only"][n - 1]
        assert set(np.unique(cases["bytes_2_255"])) == {0, 2, 255}
        if "one_chunk_hidden" in cases:
            hidden = np.flatnonzero(~cases["one_chunk_hidden"])
            assert hidden[0] == cr.CHUNK and hidden[-1] == 2 * cr.CHUNK - 1 and hidden.size == cr.CHUNK


def test_the_sizes_sit_on_the_edges_they_name():
    assert cr.CHUNK == 4096 and cr.CHUNK == 256 * 16             # 256 threads, one 16-byte load of flags each
    assert cr.CHUNK_SIZES == (cr.CHUNK - 1, cr.CHUNK, cr.CHUNK + 1, 2 * cr.CHUNK + 1)
    assert set(vr.SIZES) | set(cr.CHUNK_SIZES) == set(cr.SIZES) and list(cr.SIZES) == sorted(cr.SIZES)
    chunks = lambda n: -(-n // cr.CHUNK)
    assert [chunks(n) for n in cr.CHUNK_SIZES] == [1, 1, 2, 3]
    assert (2 * cr.CHUNK + 1) % cr.CHUNK == 1                    # the last chunk holds one splat
    assert cr.ID_NONE == _capi.ID_NONE


def test_the_map_is_an_ascending_bijection_from_the_kept_onto_0_to_k():
    for n in (1, 255, cr.CHUNK + 1):
        for name, mask in cr.mask_cases(n).items():
            keep = cr.keep_of(mask)
            m, k = cr.index_map(mask)
            assert m.dtype == np.uint32 and m.shape == (n,) and k == keep.sum(), (n, name)
            assert (m[~keep] == cr.ID_NONE).all(), (n, name)
            np.testing.assert_array_equal(m[keep], np.arange(k, dtype=np.uint32))       # ascending, dense, onto 0..K-1
            np.testing.assert_array_equal(np.flatnonzero(keep)[m[keep]], np.flatnonzero(keep))
    m, k = cr.index_map(np.array([0, 2, 0, 255, 1], np.uint8))
    assert k == 3 and m.tolist() == [cr.ID_NONE, 0, cr.ID_NONE, 1, 2]
