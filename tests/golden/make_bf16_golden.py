#!/usr/bin/env python3
"""Regenerate the BF16 fixtures (tests/golden/bf16*) from the real reference build.

Needs oracle/_ref/libggml_ref.so (`make -C oracle ref`, where the reference sources exist). Every
byte written here comes out of the reference's own functions, called through ctypes:

  bf16_convert_sample.u16   ggml_fp32_to_bf16_row over the sampled members (bf16_cases.converter_sample:
                            every zero, subnormal, inf and NaN, every 61st of the rest) of the converter's
                            input set (every upper-16-bit pattern x six lower halves)
  bf16_K*_N*_B*.y.f32       reference CPU backend MUL_MAT of bf16_cases.GOLDEN_CASES (inputs from their seeds)
  bf16.json                 the manifest: the SHA-256 of the reference's outputs over the whole converter set
                            and over all 65 536 f16 patterns (f16 -> f32 -> bf16), the set's class counts,
                            and the files above (bytes, SHA-256)

The manifests of the other golden vectors are not touched.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import bf16_cases as C  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")


def ref_to_bf16(lib, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.size, np.uint16)
    lib.ggml_fp32_to_bf16_row(x.ctypes.data, out.ctypes.data, x.size)
    return out


def main() -> None:
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    files = {}

    def put(name: str, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        a.tofile(os.path.join(HERE, name))
        files[name] = {"bytes": int(a.nbytes), "sha256": C.sha256(a)}

    u = C.converter_set()
    full = ref_to_bf16(lib, u.view(np.float32))
    put("bf16_convert_sample.u16", full[C.converter_sample(u)])
    f16 = ref_to_bf16(lib, C.f16_patterns_as_f32(lib))
    cases = {}
    for K, N, B in C.GOLDEN_CASES:
        wb, x = C.case_inputs(K, N, B)
        y = G.mul_mat_once(lib, cpu, C.BF16, C.weight_bytes(wb), K, N, x.ravel(), B)
        name = f"bf16_K{K}_N{N}_B{B}.y.f32"
        put(name, y)
        cases[name] = {"K": K, "N": N, "B": B}
    lib.ggml_backend_free(cpu)
    manifest = {
        "generator": "tests/golden/make_bf16_golden.py on oracle/_ref/libggml_ref.so",
        "converter_set": {"members": int(u.size), "low_halves": [hex(v) for v in C.LOW_HALVES], "sha256": C.sha256(full),
                          "sample_members": int(C.converter_sample(u).size), "classes": C.converter_classes(u)},
        "f16_to_bf16": {"members": 65536, "sha256": C.sha256(f16)},
        "cases": cases,
        "files": files,
    }
    with open(os.path.join(HERE, "bf16.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print(json.dumps(manifest["converter_set"]["classes"], indent=1))
    print({k: v["bytes"] for k, v in files.items()})


if __name__ == "__main__":
    main()
