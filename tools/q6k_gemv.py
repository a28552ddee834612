"""Decode GEMV throughput of quantized weight types (B = 1, grouped graphs of R rotated weights,
> 288 MiB per step): GB/s of algorithmic bytes by HIP events, for 4096x4096, 4096x11008 and
11008x4096 in tree order (mmv_order 0) and in the reference CPU's order (mmv_order 1), one line per
configuration.

  python tools/q6k_gemv.py                      Q6_K at the three shapes, and Q5_K and Q8_0 at
                                                  4096x11008 -- kernels Q6_K does not touch -- as the
                                                  yardstick of the box and the moment (kept as
                                                  profiles/q6k_gemv.txt)
  python tools/q6k_gemv.py q4_1 q5_0 q5_1 q4_0 q8_0
                                                  the named types at the three shapes each (kept as
                                                  profiles/legacy_gemv.txt)
"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
import torch  # noqa: E402

SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))
names = [a for a in sys.argv[1:]]
by_lower = {k.lower(): k for k in G.TYPE_BY_NAME}
if names:
    for a in names:
        assert a.lower() in by_lower, f"unknown type {a}: one of {sorted(by_lower)}"
    CONFIGS = tuple((by_lower[a.lower()], G.TYPE_BY_NAME[by_lower[a.lower()]], k, n) for a in names for k, n in SHAPES)
else:
    CONFIGS = tuple(("q6_K", 14, k, n) for k, n in SHAPES) + (("q5_K", 13, 4096, 11008), ("q8_0", 8, 4096, 11008))

lib = G.runtime()
be = G.mi355x_backend(lib, 0)
sp = lib.ggml_backend_mi355x_get_stream(be)
print("type  K x N (B = 1)    rotated  MiB/step  order            ms/step   GB/s (algorithmic bytes)", flush=True)
for tname, tt, k, n in CONFIGS:
    r = max(8, int(320 * 2**20 // (G.row_size(tt, k) * n)) + 1)
    w = bench.MulMatWorkload(lib, be, tt, k, n, 1, r)
    try:
        for order, oname in ((0, "tree"), (1, "reference-cpu")):
            assert lib.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
            for _ in range(3):
                w.step()
            lib.ggml_backend_synchronize(be)
            ms = min(bench.event_time_per_step(torch, w, sp, iters=10) for _ in range(3))
            nbytes = r * bench.unit_bytes(tt, k, n, 1)
            print(f"{tname}  {k:5d} x {n:5d}    {r:7d}  {r * G.row_size(tt, k) * n / 2**20:8.1f}  {oname:14s}  {ms:8.4f}  {nbytes / (ms / 1e3) / 1e9:7.1f}",
                  flush=True)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
        w.free()
lib.ggml_backend_free(be)
