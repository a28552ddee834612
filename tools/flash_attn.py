"""GGML_OP_FLASH_ATTN_EXT on MI355X by HIP events (kept as profiles/flash_attn.txt).

L independent attention layers in one graph, each with its own Q, K and V (f16 K/V, one shared f16
mask), run as a graph plan. L is chosen so that the K and V (decode) or Q, K and V (prompts) a step
reads exceed the 256 MiB of last-level cache. Each shape is timed in two forms, same commit, same run:

  fused   ggml_flash_attn_ext(Q, K, V, mask, scale, 0)
  chain   the same attention as the backend ran it before the op existed:
          mul_mat(K, Q) -> soft_max_ext(mask, scale) -> mul_mat(cont(transpose(V)), KQ)
          (nodes whose code the op's kernels do not touch)

Rounds alternate between the two forms, best of three, all three listed. A chain that the backend
refuses a node of is reported as such.

  decode   D = 128, 32 heads over 8 KV heads, N = 1 and 8 queries, kv = 512 / 4096 / 32768;
           reported: us per attention and the K + V bytes (2 kv nh_kv D 2) per second against 8 TB/s
  prompt   D = 128, 32 heads over 8 KV heads, N = kv = 512 / 2048, causal;
           reported: us per attention and 4 N kv D nh / 2 FLOP per second against 2.5 PF/s (f16 MFMA)

  python tools/flash_attn.py [decode] [prompt]
"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "ggml-imax_amd"))
import numpy as np  # noqa: E402
import bench  # noqa: E402
from ggml_mi355x import ggml as G  # noqa: E402
from ggml_mi355x import synth  # noqa: E402
import torch  # noqa: E402

F32, F16 = G.GGML_TYPE_F32, G.GGML_TYPE_F16
D, NH, NH_KV = 128, 32, 8
LLC = 256 * 2**20
lib = G.runtime()
be = sp = None


class Plan:
    def __init__(self, build, n_tensors, n_nodes):
        self.ctx = G.Context(lib, lib.ggml_tensor_overhead() * n_tensors + lib.ggml_graph_overhead_custom(n_nodes, False), no_alloc=True)
        c = self.ctx.ctx
        feeds, outs, self.refused = build(c)
        self.graph = lib.ggml_new_graph_custom(c, n_nodes, False)
        for o in outs:
            lib.ggml_build_forward_expand(self.graph, o)
        self.buf = self.plan = None
        if self.refused:
            return
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        for t, arr in feeds:
            G.tensor_set(lib, t, arr)
        assert lib.ggml_backend_graph_compute(be, self.graph) == 0  # direct once: scratch sized
        self.launches = lib.ggml_backend_mi355x_last_launch_count(be)
        self.plan = lib.ggml_backend_graph_plan_create(be, self.graph)
        assert self.plan

    def step(self):
        assert lib.ggml_backend_graph_plan_compute(be, self.plan) == 0

    def free(self):
        if self.plan:
            lib.ggml_backend_graph_plan_free(be, self.plan)
        if self.buf:
            lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


def layers(N, kv, L, fused, causal):
    rows = -(-N // G.GGML_KQ_MASK_PAD) * G.GGML_KQ_MASK_PAD
    scale = float(1.0 / np.sqrt(D))

    def build(c):
        feeds, outs, refused = [], [], []
        mask = np.zeros((rows, kv), np.float16)
        if causal:
            for i in range(N):
                mask[i, kv - N + i + 1:] = -np.inf
        mt = lib.ggml_new_tensor_2d(c, F16, kv, rows)
        feeds.append((mt, mask))
        kdata = (synth.uniform(2, D * kv * NH_KV)).astype(np.float16)
        qdata = synth.uniform(1, D * N * NH)
        for _ in range(L):
            q = lib.ggml_new_tensor_3d(c, F32, D, N, NH)
            k = lib.ggml_new_tensor_3d(c, F16, D, kv, NH_KV)
            v = lib.ggml_new_tensor_3d(c, F16, D, kv, NH_KV)
            feeds += [(q, qdata), (k, kdata), (v, kdata)]  # (the same values in every layer: timing only)
            if fused:
                nodes = [lib.ggml_flash_attn_ext(c, q, k, v, mt, scale, 0.0)]
            else:
                kq = lib.ggml_mul_mat(c, k, q)
                sm = lib.ggml_soft_max_ext(c, kq, mt, scale, 0.0)
                vt = lib.ggml_cont(c, lib.ggml_transpose(c, v))
                nodes = [kq, sm, vt, lib.ggml_mul_mat(c, vt, sm)]
            refused += [lib.ggml_op_desc(n).decode() for n in nodes if not lib.ggml_backend_supports_op(be, n)]
            outs.append(nodes[-1])
        return feeds, outs, sorted(set(refused))
    return build


def time_ms(g):
    for _ in range(3):
        g.step()
    lib.ggml_backend_synchronize(be)
    one = bench.event_time_per_step(torch, g, sp, iters=2)
    iters = int(min(200, max(2, 200.0 / max(one, 1e-3))))
    return bench.event_time_per_step(torch, g, sp, iters=iters)


def ab(N, kv, L, causal):
    global be, sp
    be = G.mi355x_backend(lib, 0)
    sp = lib.ggml_backend_mi355x_get_stream(be)
    plans = {f: Plan(layers(N, kv, L, f, causal), L * 10 + 8, L * 8 + 16) for f in (True, False)}
    res = {True: [], False: []}
    for _ in range(3):  # alternate the two forms: same box, same moment
        for f in (True, False):
            if plans[f].plan:
                res[f].append(time_ms(plans[f]))
    info = {f: (plans[f].refused, getattr(plans[f], "launches", 0)) for f in plans}
    for p in plans.values():
        p.free()
    lib.ggml_backend_free(be)
    return res, info


def report(label, res, info, L, unit_per_attention, roof, unit):
    parts = []
    for f, name in ((True, "fused"), (False, "chain")):
        if not res[f]:
            parts.append(f"{name}: refused by supports_op ({', '.join(info[f][0])})")
            continue
        best = min(res[f]) / L * 1e3  # us per attention
        rate = unit_per_attention / (best * 1e-6)
        parts.append(f"{name} {best:9.2f} us {[round(v / L * 1e3, 2) for v in res[f]]} ({info[f][1] // L} launches) "
                     f"{rate / 1e12:7.3f} {unit} = {100.0 * rate / roof:5.1f}% of {roof / 1e12:.0f}")
    tail = ""
    if res[True] and res[False]:
        spread = max(max(v) / min(v) - 1.0 for v in res.values())
        tail = f"   fused / chain {min(res[True]) / min(res[False]):.4f}   round-to-round spread {spread * 100:.2f}%"
    print(f"{label} L={L}:  " + "   ".join(parts) + tail, flush=True)


def part_decode():
    print("decode: D=128, 32 heads / 8 KV heads, mask without -inf; us per attention, best of 3; K+V bytes per second against 8 TB/s")
    for N in (1, 8):
        for kv in (512, 4096, 32768):
            kv_bytes = 2 * kv * NH_KV * D * 2
            L = LLC // kv_bytes + 1 + (LLC // kv_bytes) // 4
            res, info = ab(N, kv, L, causal=False)
            report(f"N={N} kv={kv}", res, info, L, kv_bytes, 8e12, "TB/s")


def part_prompt():
    print("prompt: D=128, 32 heads / 8 KV heads, causal, N = kv; us per attention, best of 3; 4 N kv D nh / 2 FLOP per second against 2.5 PF/s")
    for N in (512, 2048):
        in_bytes = 2 * N * NH_KV * D * 2 + N * NH * D * 4
        L = LLC // in_bytes + 2
        res, info = ab(N, N, L, causal=True)
        report(f"N=kv={N}", res, info, L, 4.0 * N * N * D * NH / 2, 2.5e15, "TF/s")


parts = sys.argv[1:] or ["decode", "prompt"]
if "decode" in parts:
    part_decode()
if "prompt" in parts:
    part_prompt()
