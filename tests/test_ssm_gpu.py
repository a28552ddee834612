"""GGML_OP_SSM_CONV / GGML_OP_SSM_SCAN on MI355X against the reference CPU backend: the same node runs
through the runtime + MI355X backend and through the reference library + its CPU backend on the same bytes
(cases and numpy evaluations: tests/ssm_cases.py).

* The conv has no transcendental: outputs and states are the reference's bits. Column 0 of the state of a
  sequence that no token writes is compared nowhere (the reference leaves it unwritten).
* The scan calls expf / log1pf, so y and the states each hold two bars (ssm_cases.check_scan):
  NMSE(device, reference CPU) <= 1e-7, and NMSE(device, f64) <= 4 * NMSE(reference CPU, f64).
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
from ssm_cases import F16, F32, I32, ConvCase, ScanCase, check_scan, run_graph

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_conv(libs, case):
    """Device and reference CPU; y and every state column the reference writes must be its bits."""
    rt, be, ref, cpu = libs
    y, st = case.split(run_graph(rt, be, case.build)["out"])
    want_y, want_st = case.split(run_graph(ref, cpu, case.build)["out"])
    _, model_st, written = case.model()
    assert np.array_equal(bits(y), bits(want_y)), f"{case.what}: {int(np.sum(bits(y) != bits(want_y)))} outputs differ"
    assert np.array_equal(bits(st[:, :, 1:]), bits(want_st[:, :, 1:])), f"{case.what}: states differ"
    for seq in sorted(written):
        assert np.array_equal(bits(st[seq, :, 0]), bits(want_st[seq, :, 0])), f"{case.what}: column 0 of sequence {seq}"
    keep = ~np.isnan(model_st)
    assert np.array_equal(bits(st[keep]), bits(model_st[keep])), case.what
    return y, st


def run_scan(libs, case):
    rt, be, ref, cpu = libs
    y, st = case.split(run_graph(rt, be, case.build)["out"])
    want_y, want_st = case.split(run_graph(ref, cpu, case.build)["out"])
    exact_y, exact_st = case.exact()
    check_scan(y, want_y, exact_y, case.what + " y")
    check_scan(st, want_st, exact_st, case.what + " states")
    return y, st


# ---- one sequence ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("n_t", [1, 2, 7, 70])
@pytest.mark.parametrize("d_inner", [64, 200])
@pytest.mark.parametrize("d_conv", [4, 3])
def test_conv(libs, d_conv, d_inner, n_t, strided):
    """200 rows: ragged against the 64-row workgroups; 70 tokens: several groups of loads ahead of the chain."""
    run_conv(libs, ConvCase(d_conv, d_inner, n_t, strided=strided, seed=100 + 10 * d_conv + n_t))


@pytest.mark.parametrize("n_t", [9, 40])
@pytest.mark.parametrize("d_conv", [2, 3, 5, 6, 7, 8])
def test_conv_other_widths(libs, d_conv, n_t):
    """Every width is a kernel instance of its own and mixes unfused and fused terms differently (2: all
    fused; 5: four and one; 8: none fused). 40 tokens: the state carried from one 16-token group into the
    next and into the ragged end."""
    run_conv(libs, ConvCase(d_conv, 72, n_t, seed=150 + d_conv))


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("n_t", [1, 2, 7, 130])
@pytest.mark.parametrize("d_inner", [64, 200])
def test_scan_d_state_16(libs, d_inner, n_t, strided):
    """The kernel stages 64 tokens at a time: 130 crosses two chunk boundaries and ends in a partial group
    of the unrolled chain; 200 rows leave the last workgroup (16 rows) half empty."""
    run_scan(libs, ScanCase(16, d_inner, n_t, strided=strided, seed=200 + n_t))


@pytest.mark.parametrize("d_state", [8, 24])
def test_scan_generic_d_state(libs, d_state):
    run_scan(libs, ScanCase(d_state, 72, 9, seed=300 + d_state))
    run_scan(libs, ScanCase(d_state, 72, 9, strided=True, seed=310 + d_state))


# ---- several sequences in one batch ------------------------------------------------------------------------

INTERLEAVED = [[0, -1, -1], [2, -1, -1]] * 3
# token 0 writes sequence 1 and copies it to 2; token 2 reads that copy; token 1's copy list stops at -1
FAN_OUT = [[1, 2, -1], [0, -1, 2], [2, -1, -1], [0, -1, -1], [1, 0, -1], [2, -1, -1]]


@pytest.mark.parametrize("d_conv", [4, 3])
def test_conv_interleaved_sequences(libs, d_conv):
    case = ConvCase(d_conv, 64, 6, n_kv=3, sq=INTERLEAVED, seed=400 + d_conv)
    _, st = run_conv(libs, case)
    assert np.array_equal(bits(st[1, :, 1:]), bits(case.s[1])), "sequence 1 is never touched"


@pytest.mark.parametrize("d_conv", [4, 3])
def test_conv_fan_out_with_early_stop(libs, d_conv):
    case = ConvCase(d_conv, 64, 6, n_kv=3, sq=FAN_OUT, seed=410 + d_conv)
    run_conv(libs, case)
    # the same tokens without the id behind the -1: the same result, so the copy stopped there
    sq = np.array(FAN_OUT, np.int32)
    sq[1, 2] = -1
    other = ConvCase(d_conv, 64, 6, n_kv=3, sq=sq, seed=410 + d_conv)
    rt, be, _, _ = libs
    a, b = run_graph(rt, be, case.build)["out"], run_graph(rt, be, other.build)["out"]
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("d_state", [16, 24])
def test_scan_interleaved_sequences(libs, d_state):
    case = ScanCase(d_state, 64, 6, n_kv=3, sq=INTERLEAVED, seed=420 + d_state)
    _, st = run_scan(libs, case)
    assert np.array_equal(bits(st[1]), bits(case.s[1])), "sequence 1 is never touched: its state is the input's bits"


@pytest.mark.parametrize("d_state", [16, 24])
def test_scan_fan_out_with_early_stop(libs, d_state):
    case = ScanCase(d_state, 64, 6, n_kv=3, sq=FAN_OUT, seed=430 + d_state)
    run_scan(libs, case)
    sq = np.array(FAN_OUT, np.int32)
    sq[1, 2] = -1
    other = ScanCase(d_state, 64, 6, n_kv=3, sq=sq, seed=430 + d_state)
    rt, be, _, _ = libs
    a, b = run_graph(rt, be, case.build)["out"], run_graph(rt, be, other.build)["out"]
    assert np.array_equal(bits(a), bits(b))


# ---- sq is read on the device --------------------------------------------------------------------------------

def _stats(rt, be):
    arr = (ctypes.c_int64 * 6)()
    assert rt.ggml_backend_mi355x_graph_stats_ex(be, arr, 6) == 6
    return list(arr)


def test_replayed_plan_follows_new_ids(libs):
    """A conv and a scan node (n_kv 2) in one graph, captured as a plan: computed, then only `sq` overwritten
    with ggml_backend_tensor_set (sequence 0 -> 1) and the plan computed again. Nothing is captured,
    instantiated, updated or launched directly between the two runs, and each result is the reference's
    for its own ids."""
    rt, _, ref, cpu = libs
    be = G.mi355x_backend(rt)  # a backend of its own: fresh counters
    n_t = 7
    ids = [np.tile(np.array([[s, -1]], np.int32), (n_t, 1)) for s in (0, 1)]
    conv = [ConvCase(4, 200, n_t, n_kv=2, sq=i, seed=500) for i in ids]
    scan = [ScanCase(16, 200, n_t, n_kv=2, sq=i, seed=510) for i in ids]

    def both(k):
        def build(L, c):
            feeds = []
            return feeds, [("conv", conv[k].node(L, c, feeds)), ("scan", scan[k].node(L, c, feeds))]
        return build

    want = [run_graph(ref, cpu, both(k)) for k in (0, 1)]
    ctx = G.Context(rt, rt.ggml_tensor_overhead() * 64 + rt.ggml_graph_overhead(), no_alloc=True)
    try:
        feeds, outs = both(0)(rt, ctx.ctx)
        g = rt.ggml_new_graph(ctx.ctx)
        for _, t in outs:
            rt.ggml_build_forward_expand(g, t)
        buf = rt.ggml_backend_alloc_ctx_tensors(ctx.ctx, be)
        assert buf
        for t, arr in feeds:
            G.tensor_set(rt, t, arr)
        plan = rt.ggml_backend_graph_plan_create(be, g)
        assert plan
        s0 = _stats(rt, be)
        assert s0[0] == 1, s0  # the plan is a capture
        got = []
        for k in (0, 1):
            G.tensor_set(rt, conv[0].sq_tensor, ids[k])
            G.tensor_set(rt, scan[0].sq_tensor, ids[k])
            assert rt.ggml_backend_graph_plan_compute(be, plan) == G.GGML_STATUS_SUCCESS
            rt.ggml_backend_synchronize(be)
            got.append({name: G.tensor_get(rt, t, np.float32) for name, t in outs})
        assert _stats(rt, be) == s0, (s0, _stats(rt, be))
        rt.ggml_backend_graph_plan_free(be, plan)
        rt.ggml_backend_buffer_free(buf)
    finally:
        ctx.free()
        rt.ggml_backend_free(be)
    for k in (0, 1):
        y, st = conv[k].split(got[k]["conv"])
        want_y, want_st = conv[k].split(want[k]["conv"])
        assert np.array_equal(bits(y), bits(want_y)), k
        assert np.array_equal(bits(st[:, :, 1:]), bits(want_st[:, :, 1:])), k
        assert np.array_equal(bits(st[k, :, 0]), bits(want_st[k, :, 0])), k
        exact_y, exact_st = scan[k].exact()
        y, st = scan[k].split(got[k]["scan"])
        want_y, want_st = scan[k].split(want[k]["scan"])
        check_scan(y, want_y, exact_y, f"replay {k} y")
        check_scan(st, want_st, exact_st, f"replay {k} states")
        assert np.array_equal(bits(st[1 - k]), bits(scan[k].s[1 - k])), "the other sequence's state is untouched"
    assert not np.array_equal(got[0]["scan"], got[1]["scan"])


# ---- supports_op -------------------------------------------------------------------------------------------

def test_supports_op(libs):
    """Asked, never computed."""
    rt, be, _, _ = libs
    with G.Context(rt, rt.ggml_tensor_overhead() * 1024, no_alloc=True) as cx:
        c = cx.ctx
        sup = lambda t: bool(rt.ggml_backend_supports_op(be, t))
        ptr = lambda t: ctypes.cast(t, ctypes.c_void_p).value

        for d_conv in range(2, 9):
            for d_inner, n_t, n_kv in ((64, 1, 1), (200, 70, 1), (64, 6, 3)):
                for strided in (False, True):
                    assert sup(ConvCase(d_conv, d_inner, n_t, n_kv=n_kv, sq=np.zeros((n_t, n_kv), np.int32), strided=strided).node(rt, c, [])), d_conv
        for d_state in (16, 8, 24, 1):
            for d_inner, n_t, n_kv in ((64, 1, 1), (200, 130, 1), (64, 6, 3)):
                for strided in (False, True):
                    assert sup(ScanCase(d_state, d_inner, n_t, n_kv=n_kv, sq=np.zeros((n_t, n_kv), np.int32), strided=strided).node(rt, c, [])), d_state
        # d_conv outside 2 .. 8
        assert not sup(ConvCase(9, 64, 2).node(rt, c, []))
        # an F16 state, a sq that is not I32: the builders refuse both, so the nodes are altered after they were built
        r = ConvCase(4, 64, 2).node(rt, c, [])
        r.contents.src[0] = ptr(rt.ggml_new_tensor_3d(c, F16, 3, 64, 1))
        assert not sup(r)
        r = ConvCase(4, 64, 2).node(rt, c, [])
        r.contents.src[3] = ptr(rt.ggml_new_tensor_2d(c, F32, 1, 2))
        assert not sup(r)
        r = ScanCase(16, 64, 2).node(rt, c, [])
        r.contents.src[0] = ptr(rt.ggml_new_tensor_3d(c, F16, 16, 64, 1))
        assert not sup(r)
        r = ScanCase(16, 64, 2).node(rt, c, [])
        r.contents.src[6] = ptr(rt.ggml_new_tensor_2d(c, F32, 1, 2))
        assert not sup(r)
        # a state in a split buffer
        split = rt.ggml_backend_mi355x_split_buffer_type(None)
        with G.Context(rt, rt.ggml_tensor_overhead() * 8, no_alloc=True) as cs:
            s = rt.ggml_new_tensor_2d(cs.ctx, F32, 16, 64)
            buf = rt.ggml_backend_alloc_ctx_tensors_from_buft(cs.ctx, split)
            assert buf
            try:
                r = ScanCase(16, 64, 2).node(rt, c, [])
                r.contents.src[0] = ptr(s)
                assert not sup(r)
            finally:
                rt.ggml_backend_buffer_free(buf)
