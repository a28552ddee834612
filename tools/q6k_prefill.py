"""Q6_K or IQ4_XS prompt mul_mats in tree order: the type's int8-MFMA GEMM (mmq_sub.hip)
against the 8-column chunks of the decode GEMV (tree_prefill_cols INT_MAX: the route every prompt of
the type took before its GEMM existed), alternated in one process. Graphs of R rotated weights (> 288
MiB per step, above the Infinity Cache), HIP events, us per mul_mat. Every setting is measured REPS
times, interleaved with the others, so the spread of one route is on the page next to the difference
between two. Q4_K at the same shapes (its default MFMA route and the same chunks) is the yardstick of
the box.

  python tools/q6k_prefill.py            (kept as profiles/q6k_prefill.txt)
  python tools/q6k_prefill.py iq4_xs     (kept as profiles/iq4xs_prefill.txt)
  python tools/q6k_prefill.py q3_K q2_K  (kept as profiles/q2k_q3k_prefill.txt)
"""
import os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
import torch  # noqa: E402

INT_MAX = 2**31 - 1
SHAPES = ((4096, 4096), (11008, 4096))
COLS = (16, 32, 64, 128, 512)
REPS = 3
# setting -> (tree_prefill_cols, mmq_variant)
SETTINGS = {"q6_K": (("default", 0, 0), ("k_mmq6p", 0, 16), ("k_mmq6x", 0, 128), ("chunks", INT_MAX, 0)),
            "iq4_xs": (("default", 0, 0), ("k_mmqi4p", 0, 16), ("k_mmqi4x", 0, 128), ("chunks", INT_MAX, 0)),
            "q3_K": (("default", 0, 0), ("k_mmq3p", 0, 16), ("k_mmq3x", 0, 128), ("chunks", INT_MAX, 0)),
            "q2_K": (("default", 0, 0), ("k_mmq2p", 0, 16), ("k_mmq2x", 0, 128), ("chunks", INT_MAX, 0)),
            "q4_K": (("default", 0, 0), ("chunks", INT_MAX, 0))}
TYPES = (sys.argv[1:] or ["q6_K"]) + ["q4_K"]
assert all(t in SETTINGS for t in TYPES), TYPES

lib = G.runtime()
be = G.mi355x_backend(lib, 0)
sp = lib.ggml_backend_mi355x_get_stream(be)


def tune(**kv):
    for k, v in kv.items():
        assert lib.ggml_backend_mi355x_set_tuning(k.encode(), v), (k, v)


print("type    K x N            B  rotated  setting   us per mul_mat: median  (each run)", flush=True)
try:
    tune(mmv_order=0)
    for tname in TYPES:
        tt = G.TYPE_BY_NAME[tname]
        for k, n in SHAPES:
            r = max(8, int(320 * 2**20 // (G.row_size(tt, k) * n)) + 1)
            for b in COLS:
                w = bench.MulMatWorkload(lib, be, tt, k, n, b, r)
                try:
                    runs = {s[0]: [] for s in SETTINGS[tname]}
                    for _ in range(REPS):
                        for name, cols, var in SETTINGS[tname]:
                            tune(tree_prefill_cols=cols, mmq_variant=var)
                            w.step()
                            lib.ggml_backend_synchronize(be)
                            runs[name].append(bench.event_time_per_step(torch, w, sp, iters=5) * 1e3 / r)
                    for name, _, _ in SETTINGS[tname]:
                        each = " ".join(f"{v:8.2f}" for v in runs[name])
                        print(f"{tname:6s}  {k:5d} x {n:5d}  {b:4d}  {r:7d}  {name:8s}  {statistics.median(runs[name]):8.2f}  ({each})",
                              flush=True)
                finally:
                    w.free()
finally:
    tune(mmv_order=-1, tree_prefill_cols=0, mmq_variant=0)
    lib.ggml_backend_free(be)
