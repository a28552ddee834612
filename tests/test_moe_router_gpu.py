"""The mixture-of-experts router on MI355X against the reference CPU backend: GGML_OP_ARGSORT and
GGML_OP_SUM_ROWS alone, the router chain (soft_max -> top-k -> get_rows -> sum_rows -> div) fused into
one launch and unfused, a whole MoE block that computes its own expert ids, and that block under graph
capture. The same graph runs through both libraries on the same bytes; everything is compared by bits.

Ties are the normal case for a router: the soft_max takes exp from an fp16 table, so distinct logits
give equal probabilities, and the reference's exchange sort (src/ggml.c:15064-15105) is not stable.
"""
import ctypes
import os

import numpy as np
import pytest

import test_mul_mat_id_gpu as M
from conftest import REPO
from ggml_mi355x import ggml as G
from ggml_mi355x import synth

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]

F32, F16, I32, Q4_K = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32, G.GGML_TYPE_Q4_K
ASC, DESC = 0, 1


@pytest.fixture(scope="module")
def libs():
    rt = G.runtime()
    be = G.mi355x_backend(rt)
    ref = G.Lib([REF_LIB], isolated=True)
    cpu = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(cpu, min(16, os.cpu_count() or 1))
    yield rt, be, ref, cpu
    ref.ggml_backend_free(cpu)
    rt.ggml_backend_free(be)


def run_graph(L, backend, build, n_tensors=64):
    """build(L, ctx) -> (feeds, outs: name -> tensor of 4-byte elements). Returns name -> uint32 array."""
    with G.Context(L, L.ggml_tensor_overhead() * n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
        feeds, outs = build(L, c.ctx)
        g = L.ggml_new_graph(c.ctx)
        for t in outs.values():
            L.ggml_build_forward_expand(g, t)
        buf = L.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return {name: G.tensor_get(L, t, np.uint32) for name, t in outs.items()}
        finally:
            L.ggml_backend_buffer_free(buf)


def both(libs, build, n_tensors=64):
    rt, be, ref, cpu = libs
    return run_graph(rt, be, build, n_tensors), run_graph(ref, cpu, build, n_tensors)


def same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int(np.sum(a != b))} of {a.size} words differ"


# ---- ARGSORT ----

def _argsort_inputs(ne0, rows, seed):
    rng = np.random.default_rng(seed)
    n = ne0 * rows
    ramp = np.tile(np.arange(ne0, dtype=np.float32), rows)
    return {
        "distinct": np.concatenate([rng.permutation(ne0) for _ in range(rows)]).astype(np.float32),
        "ties": rng.choice(np.array([-1.0, -0.0, 0.0, 0.5], np.float32), n),
        "equal": np.full(n, 0.25, np.float32),
        "ascending": ramp,
        "descending": -ramp,
    }


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0", [1, 2, 8, 60, 64, 65, 100, 1024])
def test_argsort(libs, ne0, order):
    """One wave per row up to 64 elements, one workgroup per row beyond; rows without equal values
    take the rank path, the others replay the reference's passes."""
    for kind, x in _argsort_inputs(ne0, 6, 100 + ne0).items():
        shape = (ne0, 3, 2, 1)
        if ne0 == 1024 and kind == "ties":
            shape, x = (ne0, 2, 1, 1), x[:2 * ne0]

        def build(L, c):
            a = L.ggml_new_tensor_4d(c, F32, *shape)
            return [(a, x)], {"idx": L.ggml_argsort(c, a, order)}

        got, want = both(libs, build)
        rows = want["idx"].reshape(-1, ne0).astype(np.int64)
        assert np.array_equal(np.sort(rows, axis=1), np.tile(np.arange(ne0), (rows.shape[0], 1)))  # the reference: permutations
        same_bits(got["idx"], want["idx"], f"argsort {kind} ne0={ne0} order={order}")


# ---- SUM_ROWS ----

def _decades(n, seed):
    """mixed sign, magnitudes over six decades"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 3.0, n)).astype(np.float32)


@pytest.mark.parametrize("ne0", [1, 2, 7, 64, 257, 4096])
def test_sum_rows(libs, ne0):
    x = _decades(ne0 * 12, 200 + ne0)

    def build(L, c):
        a = L.ggml_new_tensor_4d(c, F32, ne0, 3, 2, 2)
        return [(a, x)], {"sum": L.ggml_sum_rows(c, a)}

    got, want = both(libs, build)
    assert want["sum"].size == 12
    same_bits(got["sum"], want["sum"], f"sum_rows ne0={ne0}")


@pytest.mark.parametrize("ne0", [7, 257])
def test_sum_rows_strided_view(libs, ne0):
    """The source is a view of the first ne0 elements of longer rows (nb1 larger than the row)."""
    wide = ne0 + 5
    x = _decades(wide * 12, 300 + ne0)

    def build(L, c):
        a = L.ggml_new_tensor_4d(c, F32, wide, 3, 2, 2)
        nb = a.contents.nb
        v = L.ggml_view_4d(c, a, ne0, 3, 2, 2, nb[1], nb[2], nb[3], 0)
        return [(a, x)], {"sum": L.ggml_sum_rows(c, v)}

    got, want = both(libs, build)
    same_bits(got["sum"], want["sum"], f"sum_rows view ne0={ne0}")
    # (the reference really summed the short rows)
    exp = x.reshape(12, wide)[:, :ne0].astype(np.float64).sum(axis=1)
    assert np.allclose(want["sum"].view(np.float32), exp, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("ne0", [64, 4096])
def test_sum_rows_midpoint_takes_the_sequential_chain(libs, ne0):
    """[1, 2^-24, 0, ...]: the double sum is exactly the midpoint of 1.0f and its successor, so the
    interval of the parallel sum straddles a rounding boundary and one lane replays the chain. 1.0f."""
    x = np.zeros((2, ne0), np.float32)
    x[0, 0], x[0, 1] = 1.0, 2.0 ** -24
    x[1, 0], x[1, ne0 - 1] = 2.0 ** -24, 1.0

    def build(L, c):
        a = L.ggml_new_tensor_2d(c, F32, ne0, 2)
        return [(a, x)], {"sum": L.ggml_sum_rows(c, a)}

    got, want = both(libs, build)
    assert want["sum"].view(np.float32).tolist() == [1.0, 1.0]
    same_bits(got["sum"], want["sum"], "midpoint row")


# ---- the router chain from given logits ----

def build_router(L, c, logits, n_expert, k, T, tail):
    lt = L.ggml_new_tensor_2d(c, F32, n_expert, T)
    probs = L.ggml_soft_max(c, lt)
    sel = L.ggml_top_k(c, probs, k)                                            # i32 [k, T] view
    w = L.ggml_get_rows(c, L.ggml_reshape_3d(c, probs, 1, n_expert, T), sel)   # [1, k, T]
    if tail:
        w = L.ggml_reshape_2d(c, w, k, T)
        w = L.ggml_div(c, w, L.ggml_sum_rows(c, w))
    order = ctypes.cast(sel.contents.src[0], G.T)  # the argsort under the view: its first k entries per row are compared
    return [(lt, logits)], {"weights": w, "order": order, "probs": probs}


def _logits(kind, n_expert, T, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.standard_normal(n_expert * T) * 2.0).astype(np.float32)
    return (rng.integers(-16, 17, n_expert * T) / 8.0).astype(np.float32)  # multiples of 1/8 in [-2, 2], repeats


ROUTER_SHAPES = [(8, 2, 1), (8, 2, 5), (60, 4, 3), (64, 8, 12), (128, 2, 2)]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("tail", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("kind", ["random", "coarse"])
@pytest.mark.parametrize("shape", ROUTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_router_chain(libs, shape, kind, tail, fused):
    rt, be, ref, cpu = libs
    n_expert, k, T = shape
    logits = _logits(kind, n_expert, T, 7 * n_expert + T)
    build = lambda L, c: build_router(L, c, logits, n_expert, k, T, tail)
    want = run_graph(ref, cpu, build)
    if kind == "coarse":
        p = want["probs"].reshape(T, n_expert)
        assert any(len(np.unique(row)) < n_expert for row in p), "no equal probabilities: the tie path is not exercised"
    with M.tuning(rt, fuse_router=(fused, 1)):
        got = run_graph(rt, be, build)
        launches = rt.ggml_backend_mi355x_last_launch_count(be)
    assert launches == (1 if fused and n_expert <= 64 else 3 + 2 * tail), launches
    same_bits(got["probs"], want["probs"], "probs")
    same_bits(got["order"].reshape(T, n_expert)[:, :k], want["order"].reshape(T, n_expert)[:, :k], "selected experts")
    same_bits(got["weights"], want["weights"], "routing weights")


def test_router_chain_full_sort_when_the_order_has_another_reader(libs):
    """The argsort is also a graph output here: the fused kernel must write whole rows."""
    rt, be, ref, cpu = libs
    n_expert, k, T = 60, 4, 3
    logits = _logits("coarse", n_expert, T, 5)

    def build(L, c):
        feeds, outs = build_router(L, c, logits, n_expert, k, T, True)
        # a second reader of the whole argsort
        outs["rows"] = L.ggml_get_rows(c, L.ggml_reshape_3d(c, outs["probs"], 1, n_expert, T), outs["order"])
        return feeds, outs

    got, want = both(libs, build)
    for name in ("order", "weights", "rows"):
        same_bits(got[name], want[name], name)


# ---- a whole MoE block that computes its own expert ids ----
E, FF, N_EXPERT, N_USED = M.E, M.FF, M.N_EXPERT, M.N_USED


def moe_weights(t):
    return {"t": t, "gate": M.experts(t, E, FF, N_EXPERT, 31), "up": M.experts(t, E, FF, N_EXPERT, 32), "down": M.experts(t, FF, E, N_EXPERT, 33),
            "g": (1.0 + 0.1 * synth.uniform(34, E)).astype(np.float32), "gate_inp": (synth.uniform(35, E * N_EXPERT) * np.float32(0.5)).astype(np.float32)}


def build_moe_router(L, c, W, T, x, leaves=None):
    """build_moe of test_mul_mat_id_gpu with the ids and routing weights computed by the graph: the
    router of a Mixtral-style layer. leaves: a context of their own for the inputs and weights."""
    t = W["t"]
    cl = leaves or c
    xt = L.ggml_new_tensor_2d(cl, F32, E, T)
    gt = L.ggml_new_tensor_1d(cl, F32, E)
    gi = L.ggml_new_tensor_2d(cl, F32, E, N_EXPERT)
    wg = L.ggml_new_tensor_3d(cl, t, E, FF, N_EXPERT)
    wu = L.ggml_new_tensor_3d(cl, t, E, FF, N_EXPERT)
    wd = L.ggml_new_tensor_3d(cl, t, FF, E, N_EXPERT)
    h = L.ggml_mul(c, L.ggml_rms_norm(c, xt, 1e-5), gt)
    probs = L.ggml_soft_max(c, L.ggml_mul_mat(c, gi, h))                        # [N_EXPERT, T]
    sel = L.ggml_top_k(c, probs, N_USED)                                        # [N_USED, T]
    rw = L.ggml_get_rows(c, L.ggml_reshape_3d(c, probs, 1, N_EXPERT, T), sel)   # [1, N_USED, T]
    rw = L.ggml_reshape_2d(c, rw, N_USED, T)
    rw = L.ggml_div(c, rw, L.ggml_sum_rows(c, rw))
    rw = L.ggml_reshape_3d(c, rw, 1, N_USED, T)
    h3 = L.ggml_reshape_3d(c, h, E, 1, T)
    gate = L.ggml_mul_mat_id(c, wg, h3, sel)
    up = L.ggml_mul_mat_id(c, wu, h3, sel)
    down = L.ggml_mul_mat_id(c, wd, L.ggml_mul(c, L.ggml_silu(c, gate), up), sel)
    down = L.ggml_mul(c, down, rw)
    nb = down.contents.nb
    out = None
    for e in range(N_USED):
        v = L.ggml_view_2d(c, down, E, T, nb[2], e * nb[1])
        out = v if out is None else L.ggml_add(c, out, v)
    feeds = [(xt, x), (gt, W["g"]), (gi, W["gate_inp"]), (wg, W["gate"]), (wu, W["up"]), (wd, W["down"])]
    order = ctypes.cast(sel.contents.src[0], G.T)
    return feeds, {"out": out, "order": order}, xt


def _x(T, seed):
    return (synth.uniform(seed, E * T) * np.float32(2.0)).astype(np.float32)


def _selected(res, T):
    return res["order"].reshape(T, N_EXPERT)[:, :N_USED]


@pytest.mark.parametrize("T", [1, 5, 12])
def test_moe_block_with_router_q4k(libs, T):
    W = moe_weights(Q4_K)
    x = _x(T, 60 + T)
    got, want = both(libs, lambda L, c: build_moe_router(L, c, W, T, x)[0:2])
    same_bits(_selected(got, T), _selected(want, T), "selected experts")
    same_bits(got["out"], want["out"], f"MoE block T={T}")


@pytest.mark.parametrize("T", [1, 5])
def test_moe_block_with_router_f16_runs_in_reference_order(libs, T):
    """F16 experts: no quantized mul_mat asks for the reference order -- the ARGSORT of computed
    probabilities does (graph_decode_order). In tree order the output would not be the reference's bits."""
    W = moe_weights(F16)
    x = _x(T, 80 + T)
    got, want = both(libs, lambda L, c: build_moe_router(L, c, W, T, x)[0:2])
    same_bits(_selected(got, T), _selected(want, T), "selected experts")
    same_bits(got["out"], want["out"], f"F16 MoE block T={T}")


def test_moe_block_fusion_saves_four_launches(libs):
    rt, be, _, _ = libs
    W = moe_weights(Q4_K)
    x = _x(1, 61)
    n = {}
    outs = {}
    for fused in (1, 0):
        with M.tuning(rt, fuse_router=(fused, 1)):
            outs[fused] = run_graph(rt, be, lambda L, c: build_moe_router(L, c, W, 1, x)[0:2])["out"]
            n[fused] = rt.ggml_backend_mi355x_last_launch_count(be)
    print(f"MoE block with its router, T=1: {n[1]} launches fused, {n[0]} unfused")
    assert n[0] - n[1] == 4, n
    same_bits(outs[1], outs[0], "fused against unfused")


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("T", [1, 5])
def test_moe_block_in_a_graph_allocator_buffer(libs, T, fused):
    """The compute tensors share one buffer laid out by ggml_gallocr, which reuses the memory of dead
    tensors. The fused launch writes the routing weights ahead of their place in the graph, so it
    applies only where nothing live lies under them; either way the output is the reference's."""
    rt, be, ref, cpu = libs
    W = moe_weights(Q4_K)
    x = _x(T, 90 + T)
    want = run_graph(ref, cpu, lambda L, c: build_moe_router(L, c, W, T, x)[0:2])
    size = rt.ggml_tensor_overhead() * 64 + rt.ggml_graph_overhead()
    with G.Context(rt, size, no_alloc=True) as cl, G.Context(rt, size, no_alloc=True) as c, M.tuning(rt, fuse_router=(fused, 1)):
        feeds, outs, _ = build_moe_router(rt, c.ctx, W, T, x, leaves=cl.ctx)
        g = rt.ggml_new_graph(c.ctx)
        rt.ggml_build_forward_expand(g, outs["out"])
        buf = rt.ggml_backend_alloc_ctx_tensors(cl.ctx, be)
        ga = rt.ggml_gallocr_new(rt.ggml_backend_get_default_buffer_type(be))
        assert buf and ga and rt.ggml_gallocr_alloc_graph(ga, g)
        try:
            for t, arr in feeds:
                G.tensor_set(rt, t, arr)
            assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
            got = G.tensor_get(rt, outs["out"], np.uint32)
            print(f"T={T} fuse_router={fused}: {rt.ggml_backend_mi355x_last_launch_count(be)} launches, "
                  f"compute buffer {rt.ggml_gallocr_get_buffer_size(ga, 0)} bytes")
        finally:
            rt.ggml_gallocr_free(ga)
            rt.ggml_backend_buffer_free(buf)
    same_bits(got, want["out"], f"MoE block in a gallocr buffer T={T}")


def _stats(rt, be):
    arr = (ctypes.c_int64 * 6)()
    assert rt.ggml_backend_mi355x_graph_stats_ex(be, arr, 6) == 6
    return list(arr)


def test_router_under_graph_capture(libs):
    """The decode block with its router: computed, captured, then only `x` overwritten with an input
    for which other experts are selected. The capture is replayed (or updated in place) -- the launch
    sequence does not depend on the ids -- and both outputs are the reference's."""
    rt, _, ref, cpu = libs
    be = G.mi355x_backend(rt)  # a backend of its own: fresh capture cache and counters
    W = moe_weights(Q4_K)
    xa, xb = _x(1, 70), _x(1, 74)
    want = [run_graph(ref, cpu, lambda L, c: build_moe_router(L, c, W, 1, x)[0:2]) for x in (xa, xb)]
    assert not np.array_equal(_selected(want[0], 1), _selected(want[1], 1)), "the second input must select other experts"
    ctx = G.Context(rt, rt.ggml_tensor_overhead() * 64 + rt.ggml_graph_overhead(), no_alloc=True)
    try:
        feeds, outs, xt = build_moe_router(rt, ctx.ctx, W, 1, xa)
        g = rt.ggml_new_graph(ctx.ctx)
        rt.ggml_build_forward_expand(g, outs["out"])
        buf = rt.ggml_backend_alloc_ctx_tensors(ctx.ctx, be)
        assert buf
        for t, arr in feeds:
            G.tensor_set(rt, t, arr)
        s0 = _stats(rt, be)
        for _ in range(2):  # the first graph of a topology is launched directly, the second captured
            assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
        got_a = G.tensor_get(rt, outs["out"], np.uint32)
        s1 = _stats(rt, be)
        assert s1[5] - s0[5] == 1, (s0, s1)
        G.tensor_set(rt, xt, xb)
        assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
        got_b = G.tensor_get(rt, outs["out"], np.uint32)
        s2 = _stats(rt, be)
        assert s2[5] == s1[5] and s2[3] == s1[3], (s1, s2)                    # no new capture, no direct launch
        assert (s2[4] - s1[4]) + (s2[2] - s1[2]) == 1, (s1, s2)              # a replay or an in-place update
        same_bits(got_a, want[0]["out"], "first input")
        same_bits(got_b, want[1]["out"], "second input")
        rt.ggml_backend_buffer_free(buf)
    finally:
        ctx.free()
        rt.ggml_backend_free(be)


# ---- supports_op ----

def test_supports_op(libs):
    rt, be, _, _ = libs
    with G.Context(rt, rt.ggml_tensor_overhead() * 128, no_alloc=True) as cx:
        c = cx.ctx
        sup = lambda t: bool(rt.ggml_backend_supports_op(be, t))
        assert not sup(rt.ggml_argsort(c, rt.ggml_new_tensor_2d(c, F32, 1025, 2), DESC))
        assert not sup(rt.ggml_argsort(c, rt.ggml_new_tensor_2d(c, I32, 8, 2), DESC))
        assert not sup(rt.ggml_argsort(c, rt.ggml_new_tensor_2d(c, F16, 8, 2), ASC))
        assert not sup(rt.ggml_sum_rows(c, rt.ggml_new_tensor_2d(c, F16, 8, 2)))
        for ne0 in (1, 2, 8, 60, 64, 65, 100, 1024):
            for order in (ASC, DESC):
                assert sup(rt.ggml_argsort(c, rt.ggml_new_tensor_4d(c, F32, ne0, 3, 2, 1), order)), ne0
        for ne0 in (1, 2, 7, 64, 257, 4096):
            assert sup(rt.ggml_sum_rows(c, rt.ggml_new_tensor_4d(c, F32, ne0, 3, 2, 2))), ne0
