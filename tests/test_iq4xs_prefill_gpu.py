"""IQ4_XS prompts on the int8-MFMA GEMM (mmq_sub.hip: k_mmqi4p, k_mmqi4x) in tree order: the route, exact
integers from hand-made rows, the saturated ends of the integer ranges, the reference CPU, and the one
canonical fold (both shapes, grouped launches and column shards give the same bits).

Shapes: K 256 (one superblock, seven empty fold groups), 768 (three, 408-byte rows 8 mod 16), 2304 (nine:
fold groups of 2 and a ragged fifth); N 33 and 67 (ragged row tiles); B 9, 33, 68 (a ragged column
tile, a second tile, the count at which mmq_variant 16 / 128 pick either shape).

The activation quantizer (quantize_row_q8_K_reference) scales by -127 / max: a column of integers
times 2^k whose largest element is -127 * 2^k comes back exactly, d_a = 2^k. An F32 column therefore
reaches quants of -127; the -128 that |D| = 32 * 127 * 128 needs comes from hand-made Q8_K rows."""
import numpy as np
import pytest

import block_cases as bc
import weight_types as W
from ggml_mi355x import ggml as G
from ggml_mi355x import synth
from weight_types import backend, needs_ref, rt  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

WT, = W.rows("iq4xs")
T = WT.type
SHAPES = [(K, N, B) for K in (256, 768, 2304) for N in (33, 67) for B in (9, 33, 68)]
BOTH = ((16, "k_mmqi4p"), (128, "k_mmqi4x"))
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113])  # kvalues_iq4nl


def run(rt, backend, members, variant=0):
    """Independent mul_mats (wq, K, N, src1 type, src1, B) of one graph in tree order: outputs, route."""
    assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", 0) and rt.ggml_backend_mi355x_set_tuning(b"mmq_variant", variant)
    try:
        with G.Context(rt, rt.ggml_tensor_overhead() * 16 + rt.ggml_graph_overhead(), no_alloc=True) as c:
            ws = [rt.ggml_new_tensor_2d(c.ctx, T, K, N) for _, K, N, _, _, _ in members]
            xs = [rt.ggml_new_tensor_2d(c.ctx, st, K, B) for _, K, _, st, _, B in members]
            ys = W._compute(rt, backend, c, [rt.ggml_mul_mat(c.ctx, w, x) for w, x in zip(ws, xs)],
                            [(w, m[0]) for w, m in zip(ws, members)] + [(x, m[4]) for x, m in zip(xs, members)])
        return ys, rt.ggml_backend_mi355x_last_mul_mat_route(backend).decode()
    finally:
        rt.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
        rt.ggml_backend_mi355x_set_tuning(b"mmq_variant", 0)


def f32(wq, K, N, x, B):
    return (wq, K, N, G.GGML_TYPE_F32, x, B)


def iq4xs_rows(d, ls, q):
    """IQ4_XS rows from d [N, S] (fp16 values), ls [N, S, 8] (the scales ls - 32 in -32..31), q [N, S, 256] (codes 0..15)."""
    v = ls + 32
    sh = ((v >> 4) << (2 * np.arange(8))).sum(-1).astype("<u2")[..., None].view(np.uint8)
    sl = (v[..., 0::2] & 15) | ((v[..., 1::2] & 15) << 4)
    q = q.reshape(q.shape[:2] + (8, 2, 16))
    qs = (q[..., 0, :] | (q[..., 1, :] << 4)).reshape(q.shape[:2] + (128,))
    parts = [d.astype(np.float16)[..., None].view(np.uint8), sh, sl, qs]
    return np.ascontiguousarray(np.concatenate([p.astype(np.uint8) for p in parts], -1)).ravel()


def test_route(rt, backend):
    K, N = 256, 33
    for B in (9, 68):
        m = [f32(W.weights(T, K, N, 100 + K + N), K, N, synth.uniform(7, K * B), B)]
        assert run(rt, backend, m)[1].startswith("k_mmqi4")
        for variant, name in BOTH:
            assert run(rt, backend, m, variant)[1] == name


@pytest.mark.parametrize("K,N,B", SHAPES)
def test_exact_integers(rt, backend, K, N, B):
    S = K // 256
    rng = np.random.default_rng(K + N + B)
    ends = (-8, 7) if K > 768 else (-32, 31)  # both in every block, all eight scales different
    ls = np.stack([rng.permutation(np.concatenate([rng.permutation(np.arange(ends[0] + 1, ends[1]))[:6], ends]))
                   for _ in range(N * S)]).reshape(N, S, 8)
    # powers of two per row / column, doubled in every other superblock
    d = 2.0 ** (rng.integers(-6, 3, (N, 1)) + (np.arange(S) + np.arange(N)[:, None]) % 2)
    q = rng.integers(0, 16, (N, S, 256))
    amax = 1 if K > 768 else 2
    a = rng.integers(-amax, amax + 1, (B, S, 256))
    a[np.arange(B)[:, None], np.arange(S), rng.integers(0, 256, (B, S))] = -127
    da = 2.0 ** (rng.integers(-4, 4, (B, 1)) + (np.arange(S) + np.arange(B)[:, None]) % 2)
    x = (a * da[..., None]).astype(np.float32).ravel()
    wv = np.repeat(ls, 32, -1) * KVALUES[q]
    terms = np.einsum("bs,ns,nsk,bsk->bns", da, d, np.abs(wv), np.abs(a))
    # exact in every order (the ratio peaks at 0.44 of 2^24 at K 768, 0.17 at K 2304)
    assert (terms.sum(-1) / (da.min(-1)[:, None] * d.min(-1)[None, :]) < 2 ** 24).all()
    want = np.einsum("bs,ns,bns->bn", da, d, np.einsum("nsk,bsk->bns", wv, a)).astype(np.float32).ravel()
    for variant, name in BOTH:
        (y,), r = run(rt, backend, [f32(iq4xs_rows(d, ls, q), K, N, x, B)], variant)
        assert r == name
        bad = np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, bad[:8], y[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("src1", ["f32", "q8_K"])
def test_saturation(rt, backend, src1):
    K, N, B, n = 512, 8, 9, 2
    lo, hi = WT.block(0x00), WT.block(0xFF)
    pairs = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    wq = np.concatenate([np.concatenate(p) for p in pairs + pairs[::-1]])
    wv = np.array([[-32 * -127 if blk is lo else 31 * 113 for blk in p] for p in pairs + pairs[::-1]])  # (ls - 32) level, [N, n]
    if src1 == "f32":  # EXTREME_X: every quant -127 (constants, d_a = -v / 127 as the quantizer divides) or +-127
        x = np.concatenate([mk(K) for mk in W.EXTREME_X] * 3)[:K * B]
        cols = x.reshape(B, n, 256)
        v = cols[:, :, 0].astype(np.float32)
        da = (np.float32(1) / (np.float32(-127) / v)).astype(np.float64)
        aq = np.rint(cols / da[..., None]).astype(np.int64)
        st, src, reach = G.GGML_TYPE_F32, x, 32 * 127 * 127
    else:  # every quant -128
        da, aq, reach = np.full((B, n), 0.5), np.full((B, n, 256), -128), 32 * 127 * 128
        st, src = bc.Q8_K, np.concatenate([bc.q8_K(0.5, np.full(256, -128))] * (n * B))
    assert np.abs(aq).max() == (127 if src1 == "f32" else 128)
    D = aq.reshape(B, n, 8, 32).sum(-1)  # per unit of the level: D_ib = level * this
    assert np.abs(127 * D).max() == reach and np.abs(32 * 127 * D.sum(-1)).max() == 8 * 32 * reach  # D_ib, T
    Tn = wv[None, :, :] * aq.sum(-1)[:, None, :]
    want = (da[:, None, :] * Tn).sum(-1)
    bound = (n + 3) * 2.0 ** -24 * np.abs(da[:, None, :] * Tn).sum(-1)
    for variant, name in BOTH:
        (y,), r = run(rt, backend, [(wq, K, N, st, src, B)], variant)
        assert r == name
        assert (np.abs(y.reshape(B, N) - want) <= bound).all(), (name, np.abs(y.reshape(B, N) - want).max())


@needs_ref
@pytest.mark.parametrize("K,N,B", SHAPES)
def test_reference_cpu(rt, backend, K, N, B):
    m = [f32(W.weights(T, K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)]
    for variant, name in BOTH:
        (y,), r = run(rt, backend, m, variant)
        assert r == name
        assert W.rel_err(y, W._ref_mul_mat(T, K, N, B)) <= W.TREE_TOL


@pytest.mark.parametrize("K", [256, 768, 2304])
def test_one_fold(rt, backend, K):
    N, B = 67, 68
    ms = [f32(W.weights(T, K, N, 500 + i), K, N, synth.uniform(510 + i, K * B), B) for i in range(3)]
    alone = [run(rt, backend, [m], 16)[0][0] for m in ms]
    assert W.same_bits(run(rt, backend, [ms[0]], 128)[0][0], alone[0])  # k_mmqi4x against k_mmqi4p
    for variant, name in BOTH:  # grouped in one graph against each alone
        ys, r = run(rt, backend, ms, variant)
        assert r == name and all(W.same_bits(y, a) for y, a in zip(ys, alone))
    wq, x = ms[0][0], ms[0][4]
    shards = [run(rt, backend, [f32(wq, K, N, x[c0 * K:c1 * K], c1 - c0)])[0][0] for c0, c1 in ((0, 32), (32, 68))]
    assert W.same_bits(np.concatenate(shards), alone[0])
