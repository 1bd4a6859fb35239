"""CPU tests of msplat_append_cloud, no device: the entry point exists in the header, the library and the
binding -- with the header's argument list -- and refuses a NULL context; the numbering rule of tests/append_rule.py against
hand-written cases; and the fixtures of tests/test_gpu_append.py are what they claim."""
import ctypes as C
import os
import re

import numpy as np

from splatapult_amd import SplatRenderer, _capi
from tests import append_rule as ar
from tests import visibility_rule as vr
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
NONE = ar.ID_NONE
# how _capi writes the header's argument types
CTYPES = {"msplat_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint32_t*": C.c_void_p, "uint64_t": C.c_uint64,
          "uint64_t*": C.POINTER(C.c_uint64)}


def test_the_header_declares_the_call_and_the_binding_has_its_argument_list():
    header = open(HEADER).read()
    decl = ("int msplat_append_cloud(msplat_ctx* ctx, msplat_ctx* src, const uint8_t* d_select, uint64_t n, uint32_t* d_index_map, "
            "uint64_t* n_added_out);")
    assert decl in header
    assert header.index("int msplat_transform_cloud(") < header.index(decl)          # after msplat_transform_cloud
    assert hasattr(C.CDLL(_capi.LIB_PATH), "msplat_append_cloud"), "libmsplat.so does not export msplat_append_cloud"
    protos = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    assert "msplat_append_cloud" in protos, "no ctypes prototype for msplat_append_cloud"
    args = [a.strip().rsplit(" ", 1)[0] for a in re.search(r"msplat_append_cloud\((.*?)\);", decl).group(1).split(",")]
    assert protos["msplat_append_cloud"] == (C.c_int, [CTYPES[a] for a in args]), (args, protos["msplat_append_cloud"])
    assert callable(getattr(SplatRenderer, "AppendCloud", None)), "SplatRenderer has no AppendCloud"
    assert len(header.splitlines()) <= 300


def test_a_null_context_or_source_is_refused_without_a_device():
    L = _capi.lib()
    k = C.c_uint64(77)
    assert L.msplat_append_cloud(None, None, None, 0, None, C.byref(k)) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in L.msplat_last_error(None).decode()
    assert k.value == 77                                         # (nothing was written)
    assert L.msplat_append_cloud(None, None, None, 0, None, None) == _capi.ERR_INVALID_ARG


def rows(n, first):
    """n rows of 3 columns that say where they came from"""
    return np.arange(first, first + n, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)


def test_the_rule_against_hand_written_cases():
    own, src = rows(3, 0), rows(5, 100)
    # (select, the map, K, the first column of the merged rows)
    cases = [
        (np.zeros(5, bool), [NONE] * 5, 0, [0, 1, 2]),                                             # empty select
        (None, [3, 4, 5, 6, 7], 5, [0, 1, 2, 100, 101, 102, 103, 104]),                            # all
        (np.ones(5, np.uint8), [3, 4, 5, 6, 7], 5, [0, 1, 2, 100, 101, 102, 103, 104]),
        (np.array([0, 0, 1, 0, 0], bool), [NONE, NONE, 3, NONE, NONE], 1, [0, 1, 2, 102]),         # one
        (np.array([1, 0, 0, 0, 0], bool), [3, NONE, NONE, NONE, NONE], 1, [0, 1, 2, 100]),         # the first only
        (np.array([0, 0, 0, 0, 1], bool), [NONE, NONE, NONE, NONE, 3], 1, [0, 1, 2, 104]),         # the last only
        (np.array([0, 2, 0, 255, 1], np.uint8), [NONE, 3, NONE, 4, 5], 3, [0, 1, 2, 101, 103, 104]),   # any nonzero byte selects
    ]
    for select, want_map, want_k, want_rows in cases:
        m, k = ar.index_map(select, 5, 3)
        assert m.dtype == np.uint32 and m.tolist() == want_map and k == want_k, (select, m, k)
        merged = ar.merged_rows(own, src, select)
        assert merged.shape == (3 + want_k, 3) and merged[:, 0].tolist() == want_rows, (select, merged)
    # N = 0: the selection extracted into a cloud of its own
    m, k = ar.index_map(np.array([0, 1, 1, 0, 1], bool), 5, 0)
    assert m.tolist() == [NONE, 0, 1, NONE, 2] and k == 3
    assert ar.merged_rows(rows(0, 0), src, np.array([0, 1, 1, 0, 1], bool))[:, 0].tolist() == [101, 102, 104]
    # Ns = 0: nothing to append, an empty map
    for select in (None, np.zeros(0, bool)):
        m, k = ar.index_map(select, 0, 3)
        assert m.shape == (0,) and m.dtype == np.uint32 and k == 0
        assert ar.merged_rows(own, rows(0, 0), select)[:, 0].tolist() == [0, 1, 2]
    # both empty
    assert ar.index_map(None, 0, 0)[1] == 0 and ar.merged_rows(rows(0, 0), rows(0, 0), None).shape == (0, 3)


def test_the_mask_is_extended_by_k_visible_values():
    assert ar.merged_mask(None, 4) is None
    got = ar.merged_mask(np.array([0, 2, 0], np.uint8), 2)
    assert got.dtype == np.bool_ and got.tolist() == [False, True, False, True, True]
    assert ar.merged_mask(np.array([True, False]), 0).tolist() == [True, False]
    assert ar.merged_mask(np.zeros(0, bool), 3).tolist() == [True, True, True]


def test_the_map_is_an_ascending_bijection_from_the_selected_onto_n_to_n_plus_k():
    for ns in ar.SRC_SIZES:
        for n in (0, 257):
            for name, select in ar.select_cases(ns).items():
                sel = ar.picked(select, ns)
                m, k = ar.index_map(select, ns, n)
                assert m.shape == (ns,) and k == sel.sum(), (ns, name)
                assert (m[~sel] == NONE).all(), (ns, name)
                np.testing.assert_array_equal(m[sel], np.arange(n, n + k, dtype=np.uint32))


def test_the_fixtures_are_what_they_claim():
    assert ar.ID_NONE == _capi.ID_NONE and ar.WAVE == 64
    assert ar.SRC_SIZES == (1, 63, 64, 65, 4097) and ar.SRC_SIZES[-1] % ar.WAVE == 1       # a partial last wave of one splat
    for ns in ar.SRC_SIZES:
        cases = ar.select_cases(ns)
        assert cases["none"] is None and not ar.picked(cases["all_hidden"], ns).any()      # every splat, and all-zero
        assert ar.picked(cases["first_only"], ns).nonzero()[0].tolist() == [0]
        assert ar.picked(cases["last_only"], ns).nonzero()[0].tolist() == [ns - 1]
        assert ar.source_aos(ns).shape == (ns, 61) and ar.source_aos(ns, False).shape == (ns, 25)
    assert not np.array_equal(ar.source_aos(255), vr.cloud_aos(255))                       # not the destination's rows
    # the plan: every (source size, select case) pair over the four destination sizes; both orders on either side
    seen, orders = set(), set()
    for d in range(len(vr.SIZES)):
        for ns, name, own_on, src_on in ar.plan(d):
            assert name in ar.select_cases(ns), (ns, name)
            seen.add((ns, name))
            if ns == ar.SRC_SIZES[-1]:
                orders.add((own_on, src_on))
    assert seen == {(ns, name) for ns in ar.SRC_SIZES for name in ar.select_cases(ns)}
    assert orders == {(False, False), (False, True), (True, False), (True, True)}


def test_the_shim_with_append_cloud_compiles_with_gxx_and_refuses_without_a_cloud(tmp_path):
    import subprocess
    src = tmp_path / "append_shim.cpp"
    src.write_text("""
#include "splatapult_amd/host/msplat_host.hpp"
int main()
{
    SplatRenderer r, s;
    uint64_t added = 77;
    bool ok = !r.AppendCloud(s) && !r.AppendCloud(r, nullptr, nullptr, &added) && added == 77;      // no cloud (Init first)
    ok = ok && msplat_append_cloud(nullptr, nullptr, nullptr, 0, nullptr, &added) == MSPLAT_ERR_INVALID_ARG && added == 77;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "append_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], cwd=ROOT, capture_output=True, timeout=60).returncode == 0
