"""GGML_OP_MUL_MAT_ID timings on MI355X by HIP events (kept as profiles/mmid_gemv.txt).

Every graph rotates over R expert stacks (8 experts each) so that the weight bytes a step reads
exceed the 256 MiB of last-level cache; all experts hold the same quantized matrix (timing only).

(a) decode: one token, 2 of 8 experts, Q4_K and Q8_0 at K x N = 4096 x 14336 and 14336 x 4096, both
    orders. Each step is R MUL_MAT_ID nodes (one grouped k_mmv_stream launch of two members each, the
    expert looked up by the kernel), against the yardstick: the same R launches as two plain MUL_MATs
    on 2-D views of the very same expert matrices -- the unchanged kernel reading the same bytes.
    A one-element SCALE node sits between the pairs in both graphs (it keeps the plain pairs from
    merging into one launch of 2 R members); its cost is timed alone and printed.
    Q8_0 in tree order also runs the plain pair on 2-D leaves, which take the repacked copy (q80r).
(b) prompts: Q4_K 4096 x 14336, 2 of 8 experts, T tokens (b broadcast, as a gate / up projection):
    pair by pair (mmid_group 0) against grouped by expert on the device in chunks of up to 8 and of
    up to 4 pairs (mmid_group 8 / 4: grouped at any T), and for T <= 8 the streaming kernel with a
    member per pair (mmid_stream 8; 1 elsewhere in this part).

  python tools/mmid_gemv.py [a] [b]
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
N_AS, N_USED = 8, 2
lib = G.runtime()
be = G.mi355x_backend(lib, 0)
sp = lib.ggml_backend_mi355x_get_stream(be)


_quantized = {}


def quantized(t, K, N):
    """One expert's bytes; quantized once per type as rows of 4096 (the same whole blocks serve as
    K * N / 4096 rows of 4096 or as rows of any other multiple of 256)."""
    if t not in _quantized:
        f = synth.uniform(42, K * N)
        q = np.empty(G.row_size(t, 4096) * (K * N // 4096), np.uint8)
        lib.ggml_quantize_chunk(t, f.ctypes.data, q.ctypes.data, 0, K * N // 4096, 4096, None)
        _quantized[t] = q
    assert _quantized[t].nbytes == G.row_size(t, K) * N
    return _quantized[t]


class Stacks:
    """R expert stacks [K, N, 8] of type t on the device, every expert the same bytes."""

    def __init__(self, t, K, N, R, leaves=False):
        self.t, self.K, self.N, self.R = t, K, N, R
        self.ctx = G.Context(lib, lib.ggml_tensor_overhead() * (R * (1 + N_USED) + 4), no_alloc=True)
        c = self.ctx.ctx
        self.a = [lib.ggml_new_tensor_3d(c, t, K, N, N_AS) for _ in range(R)]
        self.leaf = [lib.ggml_new_tensor_2d(c, t, K, N) for _ in range(R * N_USED)] if leaves else []
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        q = quantized(t, K, N)
        self.expert_bytes = q.nbytes
        for a in self.a:
            for e in range(N_AS):
                G.tensor_set(lib, a, q, e * q.nbytes)
        for w in self.leaf:
            G.tensor_set(lib, w, q)

    def free(self):
        lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


class Graph:
    """mode 'id': R MUL_MAT_ID nodes over the stacks; 'plain' / 'leaf': per stack N_USED plain MUL_MATs
    on views of the selected experts / on 2-D leaves (T == 1); 'sep': the separators alone."""

    def __init__(self, st, mode, T, sep, seed=7):
        R, K, N = st.R, st.K, st.N
        self.ctx = G.Context(lib, lib.ggml_tensor_overhead() * (R * 12 + 8) + lib.ggml_graph_overhead_custom(R * 8 + 16, False), no_alloc=True)
        c = self.ctx.ctx
        rng = np.random.default_rng(seed)
        ids_np = [np.stack([rng.permutation(N_AS)[:N_USED] for _ in range(T)]).astype(np.int32) for _ in range(R)]
        self.graph = lib.ggml_new_graph_custom(c, R * 8 + 16, False)
        feeds = []
        for r in range(R):
            x = lib.ggml_new_tensor_3d(c, F32, K, 1, T)
            feeds.append((x, synth.uniform(seed + 1 + r, K * T)))
            if mode == "id":
                ids = lib.ggml_new_tensor_2d(c, I32, N_USED, T)
                feeds.append((ids, ids_np[r]))
                lib.ggml_build_forward_expand(self.graph, lib.ggml_mul_mat_id(c, st.a[r], x, ids))
            elif mode in ("plain", "leaf"):
                assert T == 1
                for e in range(N_USED):
                    w = st.leaf[r * N_USED + e] if mode == "leaf" else lib.ggml_view_2d(c, st.a[r], K, N, st.a[r].contents.nb[1],
                                                                                         int(ids_np[r][0, e]) * st.a[r].contents.nb[2])
                    lib.ggml_build_forward_expand(self.graph, lib.ggml_mul_mat(c, w, x))
            if sep:
                s = lib.ggml_new_tensor_1d(c, F32, 1)
                feeds.append((s, np.ones(1, np.float32)))
                lib.ggml_build_forward_expand(self.graph, lib.ggml_scale(c, s, 1.0))
        self.buf = lib.ggml_backend_alloc_ctx_tensors(c, be)
        assert self.buf, "device allocation failed"
        for t, arr in feeds:
            G.tensor_set(lib, t, arr)

    def step(self):
        assert lib.ggml_backend_graph_compute_async(be, self.graph) == 0

    def free(self):
        lib.ggml_backend_buffer_free(self.buf)
        self.ctx.free()


def tune(**kv):
    for k, v in kv.items():
        assert lib.ggml_backend_mi355x_set_tuning(k.encode(), v), (k, v)


def time_ms(g, rounds=3):
    """min over `rounds` of the event time per step; the window holds at least ~0.2 s of work or 20 steps"""
    for _ in range(3):
        g.step()
    lib.ggml_backend_synchronize(be)
    one = bench.event_time_per_step(torch, g, sp, iters=2)
    iters = int(min(20, max(2, 200.0 / max(one, 1e-3))))
    return [bench.event_time_per_step(torch, g, sp, iters=iters) for _ in range(rounds)]


def part_a():
    print("(a) decode, one token, 2 of 8 experts; R launches of two members per step; ms per step, best of 3 (all three listed)")
    print("type  K x N           R  order  variant          ms/step   [rounds]                     GB/s   id / plain")
    for tname, t in (("q4_K", 12), ("q8_0", 8)):
        for K, N in ((4096, 14336), (14336, 4096)):
            per = G.row_size(t, K) * N
            R = int(320 * 2**20 // (N_USED * per)) + 1
            st = Stacks(t, K, N, R, leaves=(t == 8))
            gs = {m: Graph(st, m, 1, True) for m in (("id", "plain", "leaf", "sep") if t == 8 else ("id", "plain", "sep"))}
            try:
                for order in (0, 1):
                    tune(mmv_order=order)
                    res = {m: [] for m in gs}
                    for _ in range(3):  # alternate the variants: same box, same moment
                        for m, g in gs.items():
                            if m == "leaf" and order == 1:
                                continue
                            res[m] += time_ms(g, rounds=1)
                    nbytes = R * N_USED * (per + 4 * K + 4 * N)
                    for m in gs:
                        if not res[m]:
                            continue
                        best = min(res[m])
                        ratio = f"{min(res['id']) / min(res['plain']):.4f}" if m == "id" else ""
                        gbs = f"{nbytes / (best / 1e3) / 1e9:7.1f}" if m != "sep" else "      -"
                        print(f"{tname}  {K:5d} x {N:5d}  {R:3d}  {order:5d}  {m:14s}  {best:8.4f}  {str([round(v, 4) for v in res[m]]):28s} {gbs}   {ratio}",
                              flush=True)
            finally:
                tune(mmv_order=-1)
                for g in gs.values():
                    g.free()
                st.free()


def part_b():
    print("(b) prompts, q4_K 4096 x 14336, 2 of 8 experts, T tokens, b broadcast; R = 3 stacks per step; ms per step, best of 3")
    print("T     order  pairwise  grouped 8  grouped 4  streaming   grouped 8 / pairwise  grouped 4 / pairwise")
    t, K, N, R = 12, 4096, 14336, 3
    st = Stacks(t, K, N, R)
    try:
        for T in (2, 8, 16, 64, 512):
            g = Graph(st, "id", T, False)
            try:
                for order in (0, 1):
                    tune(mmv_order=order)
                    res = {"pair": [], "group": [], "group4": [], "stream": []}
                    for _ in range(3):
                        tune(mmid_stream=1, mmid_group=0)
                        res["pair"] += time_ms(g, rounds=1)
                        tune(mmid_group=8)
                        res["group"] += time_ms(g, rounds=1)
                        tune(mmid_group=4)
                        res["group4"] += time_ms(g, rounds=1)
                        if T <= 8:
                            tune(mmid_stream=8)
                            res["stream"] += time_ms(g, rounds=1)
                    p, q, q4 = min(res["pair"]), min(res["group"]), min(res["group4"])
                    s = f"{min(res['stream']):9.4f}" if res["stream"] else "        -"
                    print(f"{T:4d}  {order:5d}  {p:8.4f}  {q:9.4f}  {q4:9.4f}  {s}   {q / p:20.4f}  {q4 / p:20.4f}", flush=True)
            finally:
                tune(mmv_order=-1, mmid_stream=8, mmid_group=1)
                g.free()
    finally:
        st.free()


parts = sys.argv[1:] or ["a", "b"]
if "a" in parts:
    part_a()
if "b" in parts:
    part_b()
lib.ggml_backend_free(be)
