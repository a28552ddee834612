#!/usr/bin/env python3
"""Regenerate the Q6_K fixtures (tests/golden/q6k_*) from the real reference build.

Needs oracle/_ref/libggml_ref.so (`make -C oracle ref`, where the reference sources exist). Every
byte written here comes out of the reference's own functions, called through ctypes:

  q6k_w.f32 / q6k_edge.f32        the f32 inputs (kept, so that no test depends on a generator's stream)
  q6k_w.wq.bin / q6k_edge.wq.bin  ggml_quantize_chunk(GGML_TYPE_Q6_K, imatrix = NULL)
  q6k_w.wdq.f32 / q6k_edge.wdq.f32  dequantize_row_q6_K of those blocks
  q6k_w.y.f32                     reference CPU backend mul_mat of q6k_w against B = 3 columns
  q6k.json                        the manifest of the above (shapes, seeds, SHA-256)

The manifest of the other golden vectors (manifest.json) is not touched.
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
Q6_K = 14
K_W, N_W, B_W, XSEED = 768, 8, 3, 6614
K_EDGE = 512


def edge_rows() -> tuple[np.ndarray, list[str]]:
    """The quantizer's branches, one per row of 2 superblocks."""
    rows, names = [], []

    def noise(seed, scale):
        return (synth.uniform(seed, K_EDGE) * scale).astype(np.float32)

    r = noise(601, 1.0); r[:256] = 0.0
    rows.append(r); names.append("all-zero superblock, then a normal one")
    rows.append(np.full(K_EDGE, 0.37, np.float32)); names.append("constant row")
    r = noise(602, 1e-3); r[131] = 1e4
    rows.append(r); names.append("one 1e4 outlier in 1e-3 noise")
    r = noise(603, 0.1); r[70] = 5.0; r[300] = -5.0
    rows.append(r); names.append("largest sub-block peak positive (negative scale, superblock 0) / negative (superblock 1)")
    r = noise(604, 1.0); r[48:64] = 0.0; r[256 + 240:] = 0.0
    rows.append(r); names.append("one all-zero sub-block in each superblock")
    r = noise(605, 1.0); r[16:32] *= 1e-3; r[400] = -3.0
    rows.append(r); names.append("a tiny sub-block beside large ones; a negative peak")
    return np.stack(rows), names


def main() -> int:
    ref = G.Lib([REF_LIB], isolated=True)
    G.Context(ref, 1024).free()  # the reference fills its tables in the first ggml_init
    deq = ref.handles[0].dequantize_row_q6_K
    deq.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    deq.restype = None

    def quantize(w, K):
        n = w.size // K
        out = np.empty(G.row_size(Q6_K, K) * n, np.uint8)
        w = np.ascontiguousarray(w, np.float32)
        assert ref.ggml_quantize_chunk(Q6_K, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
        back = np.empty(w.size, np.float32)
        deq(out.ctypes.data, back.ctypes.data, w.size)
        return out, back

    files = {}

    def put(name, arr):
        arr.tofile(os.path.join(HERE, name))
        files[name] = {"bytes": int(arr.nbytes), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}

    w = np.random.default_rng(6601).standard_normal(K_W * N_W).astype(np.float32)
    wq, wdq = quantize(w, K_W)
    x = synth.uniform(XSEED, K_W * B_W)
    cpu = ref.ggml_backend_cpu_init()
    try:
        y = G.mul_mat_once(ref, cpu, Q6_K, wq, K_W, N_W, x, B_W)
    finally:
        ref.ggml_backend_free(cpu)
    put("q6k_w.f32", w); put("q6k_w.wq.bin", wq); put("q6k_w.wdq.f32", wdq); put("q6k_w.y.f32", y)

    e, names = edge_rows()
    eq, edq = quantize(e.ravel(), K_EDGE)
    put("q6k_edge.f32", e.ravel()); put("q6k_edge.wq.bin", eq); put("q6k_edge.wdq.f32", edq)

    manifest = {
        "generator": "tests/golden/make_q6k_golden.py on oracle/_ref/libggml_ref.so",
        "type": Q6_K,
        "w": {"K": K_W, "N": N_W, "B": B_W, "xseed": XSEED, "x": "ggml_mi355x.synth.uniform(xseed, K * B)"},
        "edge": {"K": K_EDGE, "N": len(names), "rows": names},
        "files": files,
    }
    with open(os.path.join(HERE, "q6k.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", ", ".join(sorted(files)), "and q6k.json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
