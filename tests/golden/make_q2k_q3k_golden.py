#!/usr/bin/env python3
"""Regenerate the Q2_K / Q3_K fixtures (tests/golden/q2k_*, q3k_*) from the real reference build.

Needs oracle/_ref/libggml_ref.so (`make -C oracle ref`, where the reference sources exist). Every
byte written here comes out of the reference's own functions, called through ctypes; per type T in
(q2k, q3k):

  T_w.f32 / T_edge.f32          the f32 inputs (kept, so that no test depends on a generator's stream)
  T_w.wq.bin / T_edge.wq.bin    ggml_quantize_chunk(GGML_TYPE_Q2_K / _Q3_K, imatrix = NULL)
  T_w.wdq.f32 / T_edge.wdq.f32  dequantize_row_q2_K / _q3_K of those blocks
  T_w.y.f32                     reference CPU backend mul_mat of T_w against B = 3 columns
  q2k_q3k.json                  the manifest of the above (shapes, seeds, SHA-256)

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
TYPES = {"q2k": (10, "dequantize_row_q2_K", 2201), "q3k": (11, "dequantize_row_q3_K", 3301)}
K_W, N_W, B_W, XSEED = 768, 8, 3, 2311
K_EDGE = 512


def edge_rows() -> tuple[np.ndarray, list[str]]:
    """The quantizers' branches, one per row of 2 superblocks."""
    rows, names = [], []

    def noise(seed, scale):
        return (synth.uniform(seed, K_EDGE) * scale).astype(np.float32)

    r = noise(701, 1.0); r[:256] = 0.0
    rows.append(r); names.append("all-zero superblock, then a normal one")
    rows.append(np.full(K_EDGE, 0.37, np.float32)); names.append("constant row")
    rows.append(np.abs(noise(702, 1.0)) + 0.01); names.append("all positive (Q2_K: every min 0, dmin = 0)")
    rows.append(-np.abs(noise(703, 1.0)) - 0.01); names.append("all negative")
    r = noise(704, 1e-3); r[131] = 1e4
    rows.append(r); names.append("one 1e4 outlier in 1e-3 noise")
    r = noise(705, 0.1); r[70] = 5.0; r[300] = -5.0
    rows.append(r); names.append("largest sub-block peak positive (Q3_K: negative scale, superblock 0) / negative (superblock 1)")
    r = noise(706, 1.0); r[48:64] = 0.0; r[256 + 240:] = 0.0
    rows.append(r); names.append("one all-zero sub-block in each superblock")
    r = noise(707, 1.0); r[16:32] *= 1e-3; r[400] = -3.0
    rows.append(r); names.append("a tiny sub-block beside large ones; a negative peak")
    rows.append(noise(708, 3e-5)); names.append("values that give an fp16-subnormal d")
    return np.stack(rows), names


def main() -> int:
    ref = G.Lib([REF_LIB], isolated=True)
    G.Context(ref, 1024).free()  # the reference fills its tables in the first ggml_init
    files = {}

    def put(name, arr):
        arr.tofile(os.path.join(HERE, name))
        files[name] = {"bytes": int(arr.nbytes), "sha256": hashlib.sha256(arr.tobytes()).hexdigest()}

    e, names = edge_rows()
    x = synth.uniform(XSEED, K_W * B_W)
    manifest = {
        "generator": "tests/golden/make_q2k_q3k_golden.py on oracle/_ref/libggml_ref.so",
        "w": {"K": K_W, "N": N_W, "B": B_W, "xseed": XSEED, "x": "ggml_mi355x.synth.uniform(xseed, K * B)"},
        "edge": {"K": K_EDGE, "N": len(names), "rows": names},
        "types": {},
    }
    for tag, (t, deq_name, wseed) in TYPES.items():
        deq = getattr(ref.handles[0], deq_name)
        deq.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        deq.restype = None

        def quantize(w, K):
            n = w.size // K
            out = np.empty(G.row_size(t, K) * n, np.uint8)
            w = np.ascontiguousarray(w, np.float32)
            assert ref.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
            back = np.empty(w.size, np.float32)
            deq(out.ctypes.data, back.ctypes.data, w.size)
            return out, back

        w = np.random.default_rng(wseed).standard_normal(K_W * N_W).astype(np.float32)
        wq, wdq = quantize(w, K_W)
        cpu = ref.ggml_backend_cpu_init()
        try:
            y = G.mul_mat_once(ref, cpu, t, wq, K_W, N_W, x, B_W)
        finally:
            ref.ggml_backend_free(cpu)
        put(f"{tag}_w.f32", w); put(f"{tag}_w.wq.bin", wq); put(f"{tag}_w.wdq.f32", wdq); put(f"{tag}_w.y.f32", y)
        eq, edq = quantize(e.ravel(), K_EDGE)
        put(f"{tag}_edge.f32", e.ravel()); put(f"{tag}_edge.wq.bin", eq); put(f"{tag}_edge.wdq.f32", edq)
        manifest["types"][tag] = {"type": t, "wseed": wseed}
    manifest["files"] = files
    with open(os.path.join(HERE, "q2k_q3k.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", ", ".join(sorted(files)), "and q2k_q3k.json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
