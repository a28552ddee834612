"""CPU tests of GGML_OP_SSM_CONV / GGML_OP_SSM_SCAN on the host side (no GPU): the runtime's builders
against the reference's, and the reference CPU forwards against the numpy evaluations the GPU tests use
(tests/ssm_cases.py), which is also how the conv's rounding sequence was identified."""
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
from ssm_cases import ConvCase, ScanCase, nmse, run_graph

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference build (oracle/_ref) absent")

F32, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_I32
D_CONV, D_INNER, D_STATE, DT_RANK, N_T, N_KV = 4, 24, 16, 3, 5, 2


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def ref():
    return G.Lib([REF_LIB], isolated=True)


def _graph_signature(lib):
    """The state-space core of a Mamba layer: ssm_conv on the x half of the xz projection, its outputs as a
    view, ssm_scan with B / C as views of x_db, and the new states copied into a cache."""
    with G.Context(lib, 64 * lib.ggml_tensor_overhead() + lib.ggml_graph_overhead(), no_alloc=True) as c:
        ctx = c.ctx
        conv_s = lib.ggml_new_tensor_3d(ctx, F32, D_CONV - 1, D_INNER, N_KV)
        ssm_s = lib.ggml_new_tensor_3d(ctx, F32, D_STATE, D_INNER, N_KV)
        cache = lib.ggml_new_tensor_1d(ctx, F32, D_STATE * D_INNER * N_KV)
        xz = lib.ggml_new_tensor_2d(ctx, F32, 2 * D_INNER, N_T)
        w = lib.ggml_new_tensor_2d(ctx, F32, D_CONV, D_INNER)
        sq = lib.ggml_new_tensor_2d(ctx, I32, N_KV, N_T)
        x_db = lib.ggml_new_tensor_2d(ctx, F32, DT_RANK + 2 * D_STATE, N_T)
        dt = lib.ggml_new_tensor_2d(ctx, F32, D_INNER, N_T)
        A = lib.ggml_new_tensor_2d(ctx, F32, D_STATE, D_INNER)
        x = lib.ggml_view_2d(ctx, xz, D_INNER, N_T, xz.contents.nb[1], 0)
        conv = lib.ggml_ssm_conv(ctx, conv_s, x, w, sq)
        xc = lib.ggml_view_2d(ctx, conv, D_INNER, N_T, D_INNER * 4, 0)
        B = lib.ggml_view_2d(ctx, x_db, D_STATE, N_T, x_db.contents.nb[1], 4 * DT_RANK)
        C = lib.ggml_view_2d(ctx, x_db, D_STATE, N_T, x_db.contents.nb[1], 4 * (DT_RANK + D_STATE))
        scan = lib.ggml_ssm_scan(ctx, ssm_s, xc, dt, A, B, C, sq)
        states = lib.ggml_view_1d(ctx, scan, D_STATE * D_INNER * N_KV, D_INNER * N_T * 4)
        cpy = lib.ggml_cpy(ctx, states, lib.ggml_view_1d(ctx, cache, D_STATE * D_INNER * N_KV, 0))
        gr = lib.ggml_new_graph(ctx)
        lib.ggml_build_forward_expand(gr, cpy)
        gg = gr.contents
        sig = []
        for i in range(gg.n_nodes):
            t = gg.nodes[i].contents
            sig.append((t.op, tuple(t.ne), tuple(t.nb), tuple(t.op_params), t.type))
        nodes = {"conv": conv.contents, "scan": scan.contents}
        shapes = {k: (v.op, tuple(v.ne), v.type, [bool(s) for s in v.src]) for k, v in nodes.items()}
        return gg.n_nodes, gg.n_leafs, sig, shapes


def test_builders_shapes_and_sources(rt):
    """Both results are 1-D f32: the outputs followed by the states of every sequence (the conv's d_conv
    wide), with src[0..3] / src[0..6] set and the reference's op codes."""
    n_nodes, n_leafs, sig, shapes = _graph_signature(rt)
    assert shapes["conv"] == (G.GGML_OP_SSM_CONV, (D_INNER * N_T + D_CONV * D_INNER * N_KV, 1, 1, 1), F32, [True] * 4 + [False] * 6)
    assert shapes["scan"] == (G.GGML_OP_SSM_SCAN, (D_INNER * N_T + D_STATE * D_INNER * N_KV, 1, 1, 1), F32, [True] * 7 + [False] * 3)
    assert rt.ggml_op_name(G.GGML_OP_SSM_CONV) == b"SSM_CONV" and rt.ggml_op_name(G.GGML_OP_SSM_SCAN) == b"SSM_SCAN"
    ops = [s[0] for s in sig]
    assert ops.count(G.GGML_OP_SSM_CONV) == 1 and ops.count(G.GGML_OP_SSM_SCAN) == 1
    assert (n_nodes, n_leafs) == (9, 9)


@needs_ref
def test_graph_construction_matches_reference(rt, ref):
    assert _graph_signature(rt) == _graph_signature(ref)


# ---- the reference forwards against the numpy evaluations ------------------------------------------------

@pytest.fixture(scope="module")
def cpu(ref):
    b = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(b, 4)
    yield b
    ref.ggml_backend_free(b)


MULTI_SQ = [[1, 2, -1], [0, -1, 2], [2, -1, -1], [0, -1, -1], [1, 0, -1], [2, -1, -1]]


@needs_ref
@pytest.mark.parametrize("d_conv", [2, 3, 4, 5, 6, 7, 8])
def test_reference_conv_rounding_sequence(ref, cpu, d_conv):
    """The reference build's dot `sumf += s[i] * c[i]`: gcc vectorizes it four columns at a time (products
    and sums rounded separately, in column order) and contracts the scalar remainder into fmaf. That split,
    and no other number of leading unfused terms, reproduces its bits -- the rounding sequence the device
    kernel follows. (One leading unfused term equals none: fmaf(s, c, 0.0f) is the rounded product.)
    Multi-sequence states agree wherever the reference writes them."""
    for case in (ConvCase(d_conv, 200, 70, seed=11), ConvCase(d_conv, 64, 6, n_kv=3, sq=MULTI_SQ, seed=12)):
        y, st = case.split(run_graph(ref, cpu, case.build)["out"])
        want_y, want_st, _ = case.model()
        assert np.array_equal(y.view(np.uint32), want_y.view(np.uint32)), case.what
        keep = ~np.isnan(want_st)
        assert np.array_equal(st[keep].view(np.uint32), want_st[keep].view(np.uint32)), case.what
    case = ConvCase(d_conv, 200, 70, seed=11)
    y, _ = case.split(run_graph(ref, cpu, case.build)["out"])
    rule = 4 * (d_conv // 4)
    for k in range(2, d_conv + 1):
        if k != rule:
            other, _, _ = case.model(unfused=k)
            assert not np.array_equal(y.view(np.uint32), other.view(np.uint32)), (case.what, k)
    if rule >= 2:
        fused, _, _ = case.model(unfused=0)
        assert not np.array_equal(y.view(np.uint32), fused.view(np.uint32)), case.what


@needs_ref
@pytest.mark.parametrize("n_kv,sq", [(1, None), (3, MULTI_SQ)])
def test_reference_scan_against_f64(ref, cpu, n_kv, sq):
    """The f64 evaluation follows the reference forward, sequence handling included: f32 accuracy."""
    case = ScanCase(16, 64, 6, n_kv=n_kv, sq=sq, seed=13)
    y, st = case.split(run_graph(ref, cpu, case.build)["out"])
    want_y, want_st = case.exact()
    assert nmse(y, want_y) <= 1e-12 and nmse(st, want_st) <= 1e-12, (nmse(y, want_y), nmse(st, want_st))
