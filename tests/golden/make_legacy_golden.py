#!/usr/bin/env python3
"""Regenerate the Q4_1 / Q5_0 / Q5_1 fixtures (tests/golden/legacy_*) from the real reference build.

Needs oracle/_ref/libggml_ref.so (`make -C oracle ref`, where the reference sources exist). Every
byte written here comes out of the reference's own functions, called through ctypes:

  legacy_w.f32 / legacy_edge.f32      the f32 inputs, shared by the three types (kept, so that no test
                                      depends on a generator's stream)
  legacy_<t>_w.wq.bin / _edge.wq.bin  ggml_quantize_chunk(type, imatrix = NULL)
  legacy_<t>_w.wdq.f32 / _edge.wdq.f32  dequantize_row_<t> of those blocks
  legacy_<t>_w.y.f32                  reference CPU backend mul_mat of legacy_<t>_w against B = 3 columns
  legacy_x.xq.bin                     quantize_row_q8_1 of those B columns (block_q8_1 rows)
  legacy.json                         the manifest of the above (shapes, seeds, SHA-256)

with <t> in q4_1, q5_0, q5_1. The manifest of the other golden vectors (manifest.json) is not touched.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))

from ggml_mi355x import ggml as G  # noqa: E402
from ggml_mi355x import synth  # noqa: E402

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
TYPES = {"q4_1": 3, "q5_0": 6, "q5_1": 7}
Q8_1 = 9
K_W, N_W, B_W, XSEED = 96, 8, 3, 4151  # ragged K: three blocks a row
K_EDGE = 64


def edge_rows() -> tuple[np.ndarray, list[str]]:
    """The quantizers' branches, one per row of 2 blocks."""
    rows, names = [], []

    def noise(seed, scale):
        return (synth.uniform(seed, K_EDGE) * scale).astype(np.float32)

    r = noise(701, 1.0); r[:32] = 0.0
    rows.append(r); names.append("all-zero block, then a normal one")
    rows.append(np.full(K_EDGE, 0.37, np.float32)); names.append("constant row (min = max, d = 0 in Q4_1 / Q5_1)")
    r = noise(702, 1e-3); r[19] = 1e4
    rows.append(r); names.append("one 1e4 outlier in 1e-3 noise")
    r = noise(703, 0.1); r[7] = 5.0; r[32 + 21] = 5.0
    rows.append(r); names.append("positive peak (Q5_0: negative d), low- and high-half element")
    r = noise(704, 0.1); r[7] = -5.0; r[32 + 21] = -5.0
    rows.append(r); names.append("negative peak (Q5_0: positive d), low- and high-half element")
    r = noise(705, 0.1); r[3] = -2.0; r[9] = 2.0; r[32 + 4] = 2.0; r[32 + 30] = -2.0
    rows.append(r); names.append("+a and -a both largest: the first one decides Q5_0's sign")
    r = noise(706, 1.0); r[:32] = -1.25
    rows.append(r); names.append("a block whose min equals its max (negative constant), then a normal one")
    r = np.abs(noise(707, 1.0)) + 0.5
    rows.append(r); names.append("all positive: a non-zero min")
    return np.stack(rows), names


def main() -> int:
    ref = G.Lib([REF_LIB], isolated=True)
    G.Context(ref, 1024).free()  # the reference fills its tables in the first ggml_init

    def fn(name):
        f = getattr(ref.handles[0], name)
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        f.restype = None
        return f

    files = {}

    def put(name, arr):
        arr.tofile(os.path.join(HERE, name))
        files[name] = {"bytes": int(arr.nbytes), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}

    w = np.random.default_rng(4101).standard_normal(K_W * N_W).astype(np.float32)
    e, names = edge_rows()
    x = synth.uniform(XSEED, K_W * B_W)
    put("legacy_w.f32", w)
    put("legacy_edge.f32", e.ravel())

    xq = np.empty(G.row_size(Q8_1, K_W) * B_W, np.uint8)
    fn("quantize_row_q8_1")(x.ctypes.data, xq.ctypes.data, x.size)
    put("legacy_x.xq.bin", xq)

    cpu = ref.ggml_backend_cpu_init()
    try:
        for tname, t in TYPES.items():
            deq = fn(f"dequantize_row_{tname}")

            def quantize(v, K):
                n = v.size // K
                out = np.empty(G.row_size(t, K) * n, np.uint8)
                v = np.ascontiguousarray(v, np.float32)
                assert ref.ggml_quantize_chunk(t, v.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
                back = np.empty(v.size, np.float32)
                deq(out.ctypes.data, back.ctypes.data, v.size)
                return out, back

            wq, wdq = quantize(w, K_W)
            y = G.mul_mat_once(ref, cpu, t, wq, K_W, N_W, x, B_W)
            put(f"legacy_{tname}_w.wq.bin", wq); put(f"legacy_{tname}_w.wdq.f32", wdq); put(f"legacy_{tname}_w.y.f32", y)
            eq, edq = quantize(e.ravel(), K_EDGE)
            put(f"legacy_{tname}_edge.wq.bin", eq); put(f"legacy_{tname}_edge.wdq.f32", edq)
    finally:
        ref.ggml_backend_free(cpu)

    manifest = {
        "generator": "tests/golden/make_legacy_golden.py on oracle/_ref/libggml_ref.so",
        "types": TYPES,
        "w": {"K": K_W, "N": N_W, "B": B_W, "xseed": XSEED, "x": "ggml_mi355x.synth.uniform(xseed, K * B)"},
        "edge": {"K": K_EDGE, "N": len(names), "rows": names},
        "files": files,
    }
    with open(os.path.join(HERE, "legacy.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", ", ".join(sorted(files)), "and legacy.json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
