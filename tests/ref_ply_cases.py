"""The PLY files tests/test_host.py parses with the reference parser, and what that parser returned for them.

Where oracle/_ref/libref_ply.so was built (build() with the reference checkout present) every read goes to it and is checked
against the recorded result; elsewhere the recorded result stands in for it.  Re-record after a change to the cases:

    python -m tests.ref_ply_cases          (needs oracle/_ref/libref_ply.so)
"""
import os

import numpy as np

from oracle import oracle as orc
from splatapult_amd import synthetic
from tests.golden.make_golden import PLY_NAMES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ply_parse.npz")
ALL_NAMES = PLY_NAMES + ["nx", "ny", "nz", "a", "b", "c", "d"]

_PAY = np.arange(12, dtype="<f4").tobytes()
HEADER_CASES = {
    "ok_comments": (["ply", "comment hello", "format binary_little_endian 1.0", "comment x", "element vertex 3",
                     "property float x", "comment mid", "property float32 y", "property float z",
                     "property float opacity", "end_header"], _PAY),
    "ok_mixed_types": (["ply", "format binary_little_endian 1.0", "element vertex 1", "property uchar a",
                        "property int16 b", "property double c", "property uint d", "property float x",
                        "end_header"], bytes(19)),
    "bad_magic": (["plx", "format binary_little_endian 1.0", "element vertex 0", "end_header"], b""),
    "big_endian": (["ply", "format binary_big_endian 1.0", "element vertex 0", "end_header"], b""),
    "ascii": (["ply", "format ascii 1.0", "element vertex 0", "end_header"], b""),
    "no_element": (["ply", "format binary_little_endian 1.0", "property float x", "end_header"], b""),
    "element_face": (["ply", "format binary_little_endian 1.0", "element face 3", "end_header"], b""),
    "list_property": (["ply", "format binary_little_endian 1.0", "element vertex 1",
                       "property list uchar int vertex_indices", "end_header"], b""),
    "bad_type": (["ply", "format binary_little_endian 1.0", "element vertex 1", "property half x", "end_header"], b""),
    "not_property": (["ply", "format binary_little_endian 1.0", "element vertex 1", "element face 2",
                      "end_header"], b""),
    "truncated_header": (["ply", "format binary_little_endian 1.0", "element vertex 1", "property float x"], b""),
    "empty": ([], b""),
    "zero_vertices": (["ply", "format binary_little_endian 1.0", "element vertex 0", "property float x",
                       "end_header"], b""),
}


def write(path, header_lines, payload=b""):
    with open(path, "wb") as f:
        f.write(("\n".join(header_lines) + "\n").encode())
        f.write(payload)


def write_files(d):
    """every case file under directory d: {key: path} (test_ply = tests/golden/test.ply, synth300 = 300 synthetic splats)"""
    paths = {"test_ply": os.path.join(os.path.dirname(GOLDEN), "test.ply"), "synth300": os.path.join(str(d), "s.ply")}
    synthetic.write_ply(paths["synth300"], synthetic.generate(300, seed=5))
    for name, (hdr, payload) in HEADER_CASES.items():
        paths[name] = os.path.join(str(d), name + ".ply")
        write(paths[name], hdr, payload)
    return paths


def _recorded(key, names):
    g = np.load(GOLDEN)
    if not bool(g[key + ".meta"][0]):
        return None
    cnt, vs = int(g[key + ".meta"][1]), int(g[key + ".meta"][2])
    info = dict(zip([str(s) for s in g[key + ".pnames"]], [tuple(int(x) for x in row) for row in g[key + ".pinfo"]]))
    return cnt, vs, {n: info[n] for n in names if n in info}, g[key + ".raw"].copy()


def ref_read(key, path, names):
    """(count, vertex_size, {name: (type, size, offset)}, raw bytes) or None, as orc.ref_ply_read returns them"""
    rec = _recorded(key, names)
    if orc.ref_ply_lib() is None:
        return rec
    live = orc.ref_ply_read(path, names)
    assert (live is None) == (rec is None), key
    if live is not None:
        assert live[:3] == rec[:3], key
        np.testing.assert_array_equal(live[3], rec[3])
    return live


def record(d):
    out = {}
    for key, path in write_files(d).items():
        r = orc.ref_ply_read(path, ALL_NAMES)
        out[key + ".meta"] = np.array([r is not None, r[0] if r else 0, r[1] if r else 0], np.int64)
        props = sorted(r[2].items()) if r else []
        out[key + ".pnames"] = np.array([n for n, _ in props], dtype="<U16")
        out[key + ".pinfo"] = np.array([list(v) for _, v in props], np.int64).reshape(-1, 3)
        out[key + ".raw"] = r[3] if r else np.zeros(0, np.uint8)
    np.savez_compressed(GOLDEN, **out)


if __name__ == "__main__":
    import tempfile
    assert orc.ref_ply_lib() is not None, "oracle/_ref/libref_ply.so was not built"
    with tempfile.TemporaryDirectory() as tmp:
        record(tmp)
    print("wrote", GOLDEN)
