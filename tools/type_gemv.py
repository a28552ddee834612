"""Decode GEMV time of quantized weight types side by side (B = 1, grouped graphs of R rotated
weights, > 320 MiB per step so that no weight byte comes from the 256 MiB last-level cache), HIP
events around graph-plan steps, for 4096x4096, 4096x11008 and 11008x4096 in tree order (mmv_order 0)
and in the reference CPU's order (mmv_order 1).

The types of one shape and order are measured in alternated rounds (round 1: every type, round 2:
every type, ...), so that a drift of the box hits them alike; a line gives the median round, the
spread of the rounds (min .. max) and the GB/s of algorithmic bytes at the median.

  python tools/type_gemv.py                         Q2_K, Q3_K, Q4_K, Q6_K, IQ4_NL, IQ4_XS and Q4_0
  python tools/type_gemv.py q2_K q3_K q4_K q6_K     kept as profiles/q2k_q3k_gemv.txt
  python tools/type_gemv.py iq4_nl iq4_xs q4_0 q4_K kept as profiles/iq4_gemv.txt
  GGML_MI355X_NO_FUSED_MMV=1 python tools/type_gemv.py ...
                                                    the generic kernels (mmv.hip) serve every mul_mat:
                                                    profiles/q2k_q3k_gemv_generic.txt, iq4_gemv_generic.txt

The type column is as wide as the longest name asked for, so the lines match the kept profiles.
tools/q6k_gemv.py stays beside this script: it times one type at a time with bench.MulMatWorkload
and prints the fastest of three rounds as ms/step, other columns than these.
"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import numpy as np  # noqa: E402
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
from ggml_mi355x import synth  # noqa: E402
import torch  # noqa: E402

SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))
ROUNDS, ITERS = 5, 10
by_lower = {k.lower(): k for k in G.TYPE_BY_NAME}
names = [by_lower[a.lower()] for a in sys.argv[1:]] or ["q2_K", "q3_K", "q4_K", "q6_K", "iq4_nl", "iq4_xs", "q4_0"]
width = max(map(len, names))


class Rotated:
    """R independent B = 1 mul_mats of one graph, each with its own weight tensor. The weights are 64
    quantized rows repeated down the matrix: their values do not matter to the time."""

    def __init__(self, lib, be, t, K, N, R):
        self.lib, self.be = lib, be
        ovh = lib.ggml_tensor_overhead() * (3 * R + 8) + lib.ggml_graph_overhead_custom(4 * R + 16, False)
        self.ctx = G.Context(lib, ovh, no_alloc=True)
        c = self.ctx.ctx
        ws = [lib.ggml_new_tensor_2d(c, t, K, N) for _ in range(R)]
        xs = [lib.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, 1) for _ in range(R)]
        self.graph = lib.ggml_new_graph_custom(c, 4 * R + 16, False)
        for w, x in zip(ws, xs):
            lib.ggml_build_forward_expand(self.graph, lib.ggml_mul_mat(c, w, x))
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        wf = synth.uniform(42, K * 64)
        wq = np.empty(G.row_size(t, K) * 64, np.uint8)
        lib.ggml_quantize_chunk(t, wf.ctypes.data, wq.ctypes.data, 0, 64, K, None)
        wq = np.tile(wq, N // 64)
        for r in range(R):
            G.tensor_set(lib, ws[r], wq)
            G.tensor_set(lib, xs[r], synth.uniform(43 + r, K))

    def step(self):
        assert self.lib.ggml_backend_graph_compute_async(self.be, self.graph) == 0

    def free(self):
        self.lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


lib = G.runtime()
be = G.mi355x_backend(lib, 0)
sp = lib.ggml_backend_mi355x_get_stream(be)
print(f"# {ROUNDS} alternated rounds of {ITERS} steps per line; us per mul_mat: median (min .. max of the rounds)")
print(f"{'type':{width}s}  K x N (B = 1)    rotated  MiB/step  order           us/mul_mat median (min .. max)    GB/s (algorithmic bytes)", flush=True)
for k, n in SHAPES:
    wl = {}
    try:
        for tname in names:
            tt = G.TYPE_BY_NAME[tname]
            r = max(8, int(320 * 2**20 // (G.row_size(tt, k) * n)) + 1)
            wl[tname] = (tt, r, Rotated(lib, be, tt, k, n, r))
        for order, oname in ((0, "tree"), (1, "reference-cpu")):
            assert lib.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
            for _, _, w in wl.values():
                for _ in range(3):
                    w.step()
            lib.ggml_backend_synchronize(be)
            us = {tname: [] for tname in wl}
            for _ in range(ROUNDS):
                for tname, (tt, r, w) in wl.items():
                    us[tname].append(bench.event_time_per_step(torch, w, sp, iters=ITERS) * 1e3 / r)
            for tname, (tt, r, w) in wl.items():
                v = sorted(us[tname])
                med = v[len(v) // 2]
                gbs = bench.unit_bytes(tt, k, n, 1) / (med * 1e-6) / 1e9
                print(f"{tname:{width}s}  {k:5d} x {n:5d}    {r:7d}  {r * G.row_size(tt, k) * n / 2**20:8.1f}  {oname:14s}  "
                      f"{med:8.3f} ({v[0]:7.3f} .. {v[-1]:7.3f})         {gbs:7.1f}", flush=True)
    finally:
        lib.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
        for _, _, w in wl.values():
            w.free()
lib.ggml_backend_free(be)
