"""GGML_OP_SSM_CONV and GGML_OP_SSM_SCAN on MI355X by HIP events (kept as profiles/ssm.txt).

R independent nodes of one op in one graph, run as a graph plan: every node has its own state and its own
dst (R layers of a Mamba model, each with its states) and reads the same x / dt / A / B / C / sq, so a step
is R launches back to back and the time per node is the step over R. The states of the R nodes
(R = 32: 31 MiB of scan states in and 63 MiB out at d_inner 5120) fit the 256 MiB last-level cache, as
a model's would between two tokens.

  d_inner 5120 and 1536, d_state 16, d_conv 4, n_kv 1, n_t 1 / 8 / 64 / 512

Beside each time, the bytes the algorithm has to move and the rate they imply:
  scan  4 * (3 * d_inner * n_t + 2 * d_state * n_t + d_state * d_inner * (1 + 2 * n_kv))
  conv  4 * (2 * d_inner * n_t + d_conv * d_inner * (1 + 2 * n_kv))
Three rounds over all shapes, best and all three listed. No bar: the record is what later work is held to.

  python tools/ssm.py
"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import numpy as np  # noqa: E402
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
from ggml_mi355x import synth  # noqa: E402
import torch  # noqa: E402

F32, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_I32
D_STATE, D_CONV, N_KV, R = 16, 4, 1, 32
lib = G.runtime()
be = G.mi355x_backend(lib, 0)
sp = lib.ggml_backend_mi355x_get_stream(be)


def uniform(seed, *shape):
    return synth.uniform(seed, int(np.prod(shape))).reshape(shape).astype(np.float32)


class Plan:
    """A graph built by `build(ctx) -> (feeds, outputs)`, allocated, fed and captured as a graph plan."""

    def __init__(self, build, n_tensors, n_nodes):
        self.ctx = G.Context(lib, lib.ggml_tensor_overhead() * n_tensors + lib.ggml_graph_overhead_custom(n_nodes, False), no_alloc=True)
        c = self.ctx.ctx
        feeds, outs = build(c)
        self.graph = lib.ggml_new_graph_custom(c, n_nodes, False)
        for o in outs:
            lib.ggml_build_forward_expand(self.graph, o)
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        for t, arr in feeds:
            G.tensor_set(lib, t, arr)
        assert lib.ggml_backend_graph_compute(be, self.graph) == 0
        self.launches = lib.ggml_backend_mi355x_last_launch_count(be)
        self.plan = lib.ggml_backend_graph_plan_create(be, self.graph)
        assert self.plan

    def step(self):
        assert lib.ggml_backend_graph_plan_compute(be, self.plan) == 0

    def free(self):
        lib.ggml_backend_graph_plan_free(be, self.plan)
        lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


def conv_nodes(d_inner, n_t):
    def build(c):
        x = lib.ggml_new_tensor_2d(c, F32, d_inner, n_t)
        w = lib.ggml_new_tensor_2d(c, F32, D_CONV, d_inner)
        sq = lib.ggml_new_tensor_2d(c, I32, N_KV, n_t)
        feeds = [(x, uniform(1, n_t, d_inner)), (w, uniform(2, d_inner, D_CONV)), (sq, np.zeros((n_t, N_KV), np.int32))]
        outs = []
        for r in range(R):
            s = lib.ggml_new_tensor_3d(c, F32, D_CONV - 1, d_inner, N_KV)
            feeds.append((s, uniform(10 + r, N_KV, d_inner, D_CONV - 1)))
            outs.append(lib.ggml_ssm_conv(c, s, x, w, sq))
        return feeds, outs
    return build


def scan_nodes(d_inner, n_t):
    def build(c):
        x = lib.ggml_new_tensor_2d(c, F32, d_inner, n_t)
        dt = lib.ggml_new_tensor_2d(c, F32, d_inner, n_t)
        A = lib.ggml_new_tensor_2d(c, F32, D_STATE, d_inner)
        B = lib.ggml_new_tensor_2d(c, F32, D_STATE, n_t)
        C = lib.ggml_new_tensor_2d(c, F32, D_STATE, n_t)
        sq = lib.ggml_new_tensor_2d(c, I32, N_KV, n_t)
        a = -(np.arange(D_STATE, dtype=np.float32) + 1.0)[None, :] * (0.5 + np.abs(uniform(3, d_inner, D_STATE)))
        feeds = [(x, uniform(1, n_t, d_inner)), (dt, 1.0 + 5.0 * uniform(2, n_t, d_inner)), (A, a.astype(np.float32)),
                 (B, uniform(4, n_t, D_STATE)), (C, uniform(5, n_t, D_STATE)), (sq, np.zeros((n_t, N_KV), np.int32))]
        outs = []
        for r in range(R):
            s = lib.ggml_new_tensor_3d(c, F32, D_STATE, d_inner, N_KV)
            feeds.append((s, uniform(10 + r, N_KV, d_inner, D_STATE)))
            outs.append(lib.ggml_ssm_scan(c, s, x, dt, A, B, C, sq))
        return feeds, outs
    return build


def scan_bytes(d_inner, n_t):
    return 4 * (3 * d_inner * n_t + 2 * D_STATE * n_t + D_STATE * d_inner * (1 + 2 * N_KV))


def conv_bytes(d_inner, n_t):
    return 4 * (2 * d_inner * n_t + D_CONV * d_inner * (1 + 2 * N_KV))


def time_ms(g):
    for _ in range(3):
        g.step()
    lib.ggml_backend_synchronize(be)
    one = bench.event_time_per_step(torch, g, sp, iters=2)
    iters = int(min(200, max(2, 100.0 / max(one, 1e-3))))
    return bench.event_time_per_step(torch, g, sp, iters=iters)


SHAPES = [(d_inner, n_t) for d_inner in (5120, 1536) for n_t in (1, 8, 64, 512)]
OPS = (("ssm_scan", scan_nodes, scan_bytes), ("ssm_conv", conv_nodes, conv_bytes))

print(f"{R} nodes per graph plan, each with its own states; us per node = step / {R}; d_state {D_STATE}, d_conv {D_CONV}, n_kv {N_KV}; best of 3 rounds")
plans = {}
for op, nodes, _ in OPS:
    for shape in SHAPES:
        plans[op, shape] = Plan(nodes(*shape), 2 * R + 16, R + 16)
        assert plans[op, shape].launches == R, (op, shape, plans[op, shape].launches)
res = {k: [] for k in plans}
for _ in range(3):
    for k, p in plans.items():
        res[k].append(time_ms(p) * 1000.0 / R)
for op, _, nbytes in OPS:
    for shape in SHAPES:
        us = res[op, shape]
        b = nbytes(*shape)
        print(f"{op}  d_inner {shape[0]:5d}  n_t {shape[1]:4d}:  {min(us):9.2f} us  {[round(v, 2) for v in us]}   {b:10d} B   {b / min(us) * 1e-6:7.3f} TB/s",
              flush=True)
for p in plans.values():
    p.free()
lib.ggml_backend_free(be)
