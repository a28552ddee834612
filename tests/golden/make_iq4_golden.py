#!/usr/bin/env python3
"""Regenerate the IQ4_NL / IQ4_XS fixtures (tests/golden/iq4nl_*, iq4xs_*) from the real reference build.

Needs oracle/_ref/libggml_ref.so (`make -C oracle ref`, where the reference sources exist). Every
byte written here comes out of the reference's own functions, called through ctypes; per type T in
(iq4nl, iq4xs):

  T_w.f32 / T_edge.f32          the f32 inputs (kept, so that no test depends on a generator's stream)
  T_w.wq.bin / T_edge.wq.bin    ggml_quantize_chunk(GGML_TYPE_IQ4_NL / _IQ4_XS, imatrix = NULL)
  T_w.wdq.f32 / T_edge.wdq.f32  dequantize_row_iq4_nl / _iq4_xs of those blocks
  T_w.y.f32                     reference CPU backend mul_mat of T_w against B = 3 columns
  iq4.json                      the manifest of the above (shapes, seeds, SHA-256)

The manifests of the other golden vectors are not touched.
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
TYPES = {"iq4nl": (20, "dequantize_row_iq4_nl", 4401), "iq4xs": (23, "dequantize_row_iq4_xs", 4501)}
K_W, N_W, B_W, XSEED = 768, 8, 3, 2411
K_EDGE = 512
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float32)


def edge_rows() -> tuple[np.ndarray, list[str]]:
    """The quantizers' branches, one per row of 2 superblocks (16 blocks of 32)."""
    rows, names = [], []

    def noise(seed, scale):
        return (synth.uniform(seed, K_EDGE) * scale).astype(np.float32)

    r = noise(711, 1.0); r[:256] = 0.0
    rows.append(r); names.append("all-zero superblock (IQ4_XS: d = -0.0, scales_h 0xAAAA, codes 8), then a normal one")
    rows.append(np.full(K_EDGE, 0.37, np.float32)); names.append("constant row")
    rows.append(np.abs(noise(712, 1.0)) + 0.01); names.append("all positive")
    rows.append(-np.abs(noise(713, 1.0)) - 0.01); names.append("all negative")
    r = noise(714, 1e-3); r[131] = 1e4
    rows.append(r); names.append("one 1e4 outlier in 1e-3 noise")
    r = noise(715, 0.1); r[70] = 5.0; r[300] = -5.0
    rows.append(r); names.append("block peak positive in superblock 0, negative in superblock 1 (the sign of d)")
    r = noise(716, 1.0); r[64:96] = 0.0; r[256 + 224:] = 0.0
    rows.append(r); names.append("one all-zero 32-block in each superblock")
    r = noise(717, 1.0); r[32:64] *= 1e-3; r[400] = -3.0
    rows.append(r); names.append("a sub-block 1e-3 times its neighbours (IQ4_XS: l = 0, codes 8)")
    r = noise(718, 1e-2); r[96:128] *= 3e3; r[256 + 160:256 + 192] *= -3e3
    rows.append(r); names.append("one sub-block far larger than the rest (IQ4_XS: the others' l near 0, the clamp at -32 / 31)")
    rows.append(noise(719, 3e-3)); names.append("values that give an fp16-subnormal d (IQ4_NL about 2e-5, IQ4_XS about 7e-7)")
    r = np.tile(np.concatenate([KVALUES, KVALUES[::-1]]) * np.float32(0.01), K_EDGE // 32).astype(np.float32)
    rows.append(r); names.append("kvalues and its reverse times 0.01, tiled: all sixteen codes in both nibble halves")
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
        "generator": "tests/golden/make_iq4_golden.py on oracle/_ref/libggml_ref.so",
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
    with open(os.path.join(HERE, "iq4.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", ", ".join(sorted(files)), "and iq4.json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
