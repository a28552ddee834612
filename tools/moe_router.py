"""The mixture-of-experts router on MI355X by HIP events (kept as profiles/moe_router.txt).

One decode token through R MoE layers chained in one graph (each layer: rms_norm, mul, the router --
mul_mat(gate_inp), soft_max, top-k, get_rows, sum_rows, div --, gate / up / down MUL_MAT_ID over Q4_K
experts, silu, mul, the weighted sum of the used experts), run as a graph plan. R is chosen so that the
expert bytes a step reads exceed the 256 MiB of last-level cache; all experts hold the same quantized
matrix (timing only, the ids are whatever the router computes).

  block   E = 4096, FF = 14336, 8 experts, 2 used (Mixtral-shaped);  E = 4096, FF = 1536, 64 experts, 8 used
  chain   the router chain alone from given logits, `reps` independent chains per graph

Each is timed with the router chain fused into one launch (fuse_router 1) and as its five nodes
(fuse_router 0): same commit, same run, rounds alternated, best of three (all three listed).

  python tools/moe_router.py [block] [chain]
"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import numpy as np  # noqa: E402
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
from ggml_mi355x import synth  # noqa: E402
import torch  # noqa: E402

F32, Q4_K = G.GGML_TYPE_F32, G.GGML_TYPE_Q4_K
lib = G.runtime()
be = sp = None  # a backend per A/B pair (ab): its capture bookkeeping starts fresh


def tune(**kv):
    for k, v in kv.items():
        assert lib.ggml_backend_mi355x_set_tuning(k.encode(), v), (k, v)


class Plan:
    """A graph built by `build(ctx) -> (feeds, outputs)`, allocated, fed and captured as a graph plan
    under the tuning in force."""

    def __init__(self, build, n_tensors, n_nodes):
        self.ctx = G.Context(lib, lib.ggml_tensor_overhead() * n_tensors + lib.ggml_graph_overhead_custom(n_nodes, False), no_alloc=True)
        c = self.ctx.ctx
        feeds, outs = build(c)
        self.graph = lib.ggml_new_graph_custom(c, n_nodes, False)
        for o in outs:
            lib.ggml_build_forward_expand(self.graph, o)
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        for t, arr, off in feeds:
            G.tensor_set(lib, t, arr, off)
        assert lib.ggml_backend_graph_compute(be, self.graph) == 0  # direct once: scratch sized, tables built
        self.launches = lib.ggml_backend_mi355x_last_launch_count(be)
        self.plan = lib.ggml_backend_graph_plan_create(be, self.graph)
        assert self.plan

    def step(self):
        assert lib.ggml_backend_graph_plan_compute(be, self.plan) == 0

    def free(self):
        lib.ggml_backend_graph_plan_free(be, self.plan)
        lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


def router(c, logits, n_expert, k, T):
    probs = lib.ggml_soft_max(c, logits)
    sel = lib.ggml_top_k(c, probs, k)
    w = lib.ggml_get_rows(c, lib.ggml_reshape_3d(c, probs, 1, n_expert, T), sel)
    w = lib.ggml_reshape_2d(c, w, k, T)
    return sel, lib.ggml_div(c, w, lib.ggml_sum_rows(c, w))


def moe_layers(E, FF, n_expert, n_used, R, q_up, q_down):
    def build(c):
        feeds = []
        x = lib.ggml_new_tensor_2d(c, F32, E, 1)
        feeds.append((x, synth.uniform(3, E), 0))
        cur = x
        for r in range(R):
            g = lib.ggml_new_tensor_1d(c, F32, E)
            gi = lib.ggml_new_tensor_2d(c, F32, E, n_expert)
            wg = lib.ggml_new_tensor_3d(c, Q4_K, E, FF, n_expert)
            wu = lib.ggml_new_tensor_3d(c, Q4_K, E, FF, n_expert)
            wd = lib.ggml_new_tensor_3d(c, Q4_K, FF, E, n_expert)
            feeds.append((g, np.ones(E, np.float32), 0))
            feeds.append((gi, synth.uniform(10 + r, E * n_expert) * np.float32(0.5), 0))
            for e in range(n_expert):
                feeds += [(wg, q_up, e * q_up.nbytes), (wu, q_up, e * q_up.nbytes), (wd, q_down, e * q_down.nbytes)]
            h = lib.ggml_mul(c, lib.ggml_rms_norm(c, cur, 1e-5), g)
            sel, w = router(c, lib.ggml_mul_mat(c, gi, h), n_expert, n_used, 1)
            h3 = lib.ggml_reshape_3d(c, h, E, 1, 1)
            gate = lib.ggml_mul_mat_id(c, wg, h3, sel)
            up = lib.ggml_mul_mat_id(c, wu, h3, sel)
            down = lib.ggml_mul_mat_id(c, wd, lib.ggml_mul(c, lib.ggml_silu(c, gate), up), sel)
            down = lib.ggml_mul(c, down, lib.ggml_reshape_3d(c, w, 1, n_used, 1))
            nb = down.contents.nb
            out = None
            for e in range(n_used):
                v = lib.ggml_view_2d(c, down, E, 1, nb[2], e * nb[1])
                out = v if out is None else lib.ggml_add(c, out, v)
            cur = out
        return feeds, [cur]
    return build


def chains(n_expert, k, T, reps):
    def build(c):
        feeds, outs = [], []
        for r in range(reps):
            lt = lib.ggml_new_tensor_2d(c, F32, n_expert, T)
            feeds.append((lt, synth.uniform(20 + r, n_expert * T) * np.float32(4.0), 0))
            outs.append(router(c, lt, n_expert, k, T)[1])
        return feeds, outs
    return build


def time_ms(g):
    for _ in range(3):
        g.step()
    lib.ggml_backend_synchronize(be)
    one = bench.event_time_per_step(torch, g, sp, iters=2)
    iters = int(min(200, max(2, 200.0 / max(one, 1e-3))))
    return bench.event_time_per_step(torch, g, sp, iters=iters)


def ab(build, n_tensors, n_nodes):
    global be, sp
    be = G.mi355x_backend(lib, 0)
    sp = lib.ggml_backend_mi355x_get_stream(be)
    plans = {}
    for f in (1, 0):
        tune(fuse_router=f)
        plans[f] = Plan(build, n_tensors, n_nodes)
    res = {1: [], 0: []}
    for _ in range(3):  # alternate the two forms: same box, same moment
        for f in (1, 0):
            tune(fuse_router=f)  # (a plan that was not captured launches its nodes under the tuning in force)
            res[f].append(time_ms(plans[f]))
    tune(fuse_router=1)
    launches = {f: plans[f].launches for f in plans}
    for p in plans.values():
        p.free()
    lib.ggml_backend_free(be)
    return res, launches


def report(label, res, launches):
    b1, b0 = min(res[1]), min(res[0])
    spread = max(max(v) / min(v) - 1.0 for v in res.values())
    print(f"{label}  fused {b1:8.4f} ms {[round(v, 4) for v in res[1]]} ({launches[1]} launches)   unfused {b0:8.4f} ms "
          f"{[round(v, 4) for v in res[0]]} ({launches[0]} launches)   fused / unfused {b1 / b0:.4f}   round-to-round spread {spread * 100:.2f}%",
          flush=True)


def quantized(K, N):
    f = synth.uniform(42, K * N)
    q = np.empty(G.row_size(Q4_K, K) * N, np.uint8)
    lib.ggml_quantize_chunk(Q4_K, f.ctypes.data, q.ctypes.data, 0, N, K, None)
    return q


def part_block():
    print("block: one token through R chained MoE layers as a graph plan; ms per step, best of 3")
    for E, FF, n_expert, n_used in ((4096, 14336, 8, 2), (4096, 1536, 64, 8)):
        per_layer = 3 * n_used * G.row_size(Q4_K, E) * FF
        R = int(320 * 2**20 // per_layer) + 1
        q_up = quantized(E, FF)
        q_down = q_up  # the same whole superblocks serve as FF-long rows (timing only)
        res, launches = ab(moe_layers(E, FF, n_expert, n_used, R, q_up, q_down), R * 48 + 8, R * 40 + 16)
        report(f"E={E} FF={FF} {n_used} of {n_expert} experts, R={R} layers, {R * per_layer / 2**20:.0f} MiB of experts per step:", res, launches)


def part_chain():
    print("chain: the router chain alone from given logits (soft_max, argsort, get_rows, sum_rows, div), 16 chains per graph; ms per step, best of 3")
    for n_expert, k, T in ((8, 2, 1), (64, 8, 1), (8, 2, 512), (64, 8, 512)):
        res, launches = ab(chains(n_expert, k, T, 16), 16 * 12 + 8, 16 * 12 + 16)
        report(f"{n_expert} experts, {k} used, T={T}:", res, launches)


parts = sys.argv[1:] or ["block", "chain"]
if "block" in parts:
    part_block()
if "chain" in parts:
    part_chain()
