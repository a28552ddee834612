"""Q2_K and Q3_K prompts on the int8-MFMA GEMM (mmq_sub.hip: k_mmq2p / k_mmq2x, k_mmq3p / k_mmq3x) in tree order:
the route, exact integers from hand-made rows, the saturated ends of the integer ranges, the reference CPU,
and the one canonical fold. Shapes as test_q6k_prefill_gpu.py: K 256 (one superblock), 768 (three: Q3_K rows
2 mod 4), 2304 (nine: fold groups of 2 and a ragged fifth); N 33, 67; B 9, 33, 68; both kernel shapes.

Exact columns are integers times 2^k whose largest element is -127 * 2^k, which quantize_row_q8_K returns
as they are. Every third column is shifted by -18 and every third by +18, so the 8-byte sums P of Q2_K's
mins term pass -128 and +127 and both int8 parts of P = 128 (P >> 7) + (P & 127) carry."""
import numpy as np
import pytest

import block_cases as bc
import weight_types as W
from ggml_mi355x import ggml as G
from ggml_mi355x import synth
from weight_types import backend, needs_ref, rt  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("wt", W.rows("q2k_q3k"), ids=lambda wt: wt.tag)
SHAPES = [(K, N, B) for K in (256, 768, 2304) for N in (33, 67) for B in (9, 33, 68)]


def both(wt):
    return ((16, f"k_mmq{wt.tag[1]}p"), (128, f"k_mmq{wt.tag[1]}x"))


def run(rt, backend, T, members, variant=0, order=0):
    """Independent mul_mats (wq, K, N, src1 type, src1, B) of one graph: outputs, route."""
    assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", order) and rt.ggml_backend_mi355x_set_tuning(b"mmq_variant", variant)
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


def exact_case(wt, K, N, B):
    """Hand-made rows and columns: (weight bytes, f32 columns, the f64 result, its sum of magnitudes in units of the smallest product)."""
    S, q3 = K // 256, wt.tag == "q3k"
    rng = np.random.default_rng(K + N + B)
    raw = rng.integers(0, 256, (N, S, wt.block_bytes), dtype=np.uint8)  # qs, hmask: random bytes
    d = 2.0 ** (rng.integers(-6, 3, (N, 1)) + (np.arange(S) + np.arange(N)[:, None]) % 2)
    dmin = d * 2.0 ** rng.integers(-1, 2, (N, 1)) * (not q3)
    perm16 = lambda: np.stack([rng.permutation(16) for _ in range(N * S)]).reshape(N, S, 16)  # noqa: E731
    qs = raw[..., wt.fields["qs"]]
    qs[..., 0], qs[..., 1] = 0x00, 0xFF  # both ends of the levels in every block
    lev = ((qs.reshape(N, S, 2, 1, 32) >> (2 * np.arange(4))[:, None]) & 3).astype(np.int64)
    if q3:
        raw[..., 0], raw[..., 1] = 0x00, 0xFF
        hbit = (raw[..., wt.fields["hmask"]][:, :, None, None, :] >> (4 * np.arange(2)[:, None, None] + np.arange(4)[:, None])) & 1
        lev = lev - 4 * (1 - hbit)
        sc = np.stack([rng.permutation(np.concatenate([rng.permutation(np.arange(-31, 31))[:14], (-32, 31)])) for _ in range(N * S)]).reshape(N, S, 16)
        mn, s6 = 0 * sc, sc + 32
        hi = (s6 >> 4).reshape(N, S, 4, 4)  # [g, k]: sub-block 4g + k
        raw[..., wt.fields["scales"]] = np.concatenate([(s6[..., :8] & 15) | ((s6[..., 8:] & 15) << 4), (hi << (2 * np.arange(4))[:, None]).sum(2)], -1)
    else:
        sc, mn = perm16(), perm16()
        raw[..., wt.fields["scales"]] = sc | (mn << 4)
        raw[..., wt.fields["dmin"]] = dmin.astype(np.float16)[..., None].view(np.uint8)
    raw[..., wt.fields["d"]] = d.astype(np.float16)[..., None].view(np.uint8)
    a = rng.integers(-2, 3, (B, S, 256)) + (18 * (np.arange(B) % 3 - 1))[:, None, None]
    a[np.arange(B)[:, None], np.arange(S), rng.integers(0, 256, (B, S))] = -127
    da = 2.0 ** (rng.integers(-4, 4, (B, 1)) + (np.arange(S) + np.arange(B)[:, None]) % 2)
    wv, mv = np.repeat(sc, 16, -1) * lev.reshape(N, S, 256), np.repeat(mn, 16, -1)
    mags = np.einsum("bs,ns,nsk,bsk->bn", da, d, np.abs(wv), np.abs(a)) + np.einsum("bs,ns,nsk,bsk->bn", da, dmin, mv, np.abs(a))
    unit = da.min(-1)[:, None] * np.where(q3, d, np.minimum(d, dmin)).min(-1)[None, :]
    want = np.einsum("bs,bns->bn", da, d * np.einsum("nsk,bsk->bns", wv, a) - dmin * np.einsum("nsk,bsk->bns", mv, a))
    return raw.ravel(), (a * da[..., None]).astype(np.float32).ravel(), want.astype(np.float32).ravel(), (mags / unit).max(), a


def saturation_case(wt, src1, K=512, N=8, B=9):
    """Saturated rows against saturated columns: (weight bytes, src1 type, src1, the integer result, its bound)."""
    n, lo, hi = K // 256, wt.block(0x00), wt.block(0xFF)
    pairs = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    cT, cU = {"q2k": ((0, 45), (0, 15)), "q3k": ((128, 93), (0, 0))}[wt.tag]  # sc level and min of a 0x00 / 0xFF block
    coef = np.array([[cT[blk is hi] - cU[blk is hi] for blk in p] for p in pairs + pairs[::-1]])
    mag = np.array([[cT[blk is hi] + cU[blk is hi] for blk in p] for p in pairs + pairs[::-1]])
    if src1 == "f32":  # EXTREME_X: every quant -127 (constants, d_a = -v / 127 as the quantizer divides) or +-127
        x = np.concatenate([mk(K) for mk in W.EXTREME_X] * 3)[:K * B]
        cols = x.reshape(B, n, 256)
        da = (np.float32(1) / (np.float32(-127) / cols[:, :, 0].astype(np.float32))).astype(np.float64)
        aq, st, src = np.rint(cols / da[..., None]).astype(np.int64), G.GGML_TYPE_F32, x
    else:  # every quant -128
        da, aq = np.full((B, n), 0.5), np.full((B, n, 256), -128)
        st, src = bc.Q8_K, np.concatenate([bc.q8_K(0.5, np.full(256, -128))] * (n * B))
    assert np.abs(aq).max() == (127 if src1 == "f32" else 128)
    wq, A = np.concatenate([np.concatenate(p) for p in pairs + pairs[::-1]]), da[:, None, :] * aq.sum(-1)[:, None, :]
    return wq, st, src, (coef * A).sum(-1), (n + 3) * 2.0 ** -24 * np.abs(mag * A).sum(-1)


@ROWS
def test_route(rt, backend, wt):
    K, N = 256, 33
    for B in (9, 68):
        m = [f32(W.weights(wt.type, K, N, 100 + K + N), K, N, synth.uniform(7, K * B), B)]
        assert run(rt, backend, wt.type, m)[1].startswith(f"k_mmq{wt.tag[1]}")
        for variant, name in both(wt):
            assert run(rt, backend, wt.type, m, variant)[1] == name
        assert not run(rt, backend, wt.type, m, order=1)[1].startswith("k_mmq")


@ROWS
@pytest.mark.parametrize("K,N,B", SHAPES)
def test_exact_integers(rt, backend, wt, K, N, B):
    wq, x, want, mags, a = exact_case(wt, K, N, B)
    assert mags < 2 ** 24  # exact in every order
    P = a.reshape(B, -1, 2, 8).sum(-1)
    assert P.min() < -128 and P.max() > 127
    for variant, name in both(wt):
        (y,), r = run(rt, backend, wt.type, [f32(wq, K, N, x, B)], variant)
        assert r == name
        bad = np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, bad[:8], y[bad[:4]], want[bad[:4]])


@ROWS
@pytest.mark.parametrize("src1", ["f32", "q8_K"])
def test_saturation(rt, backend, wt, src1):
    wq, st, src, want, bound = saturation_case(wt, src1)
    for variant, name in both(wt):
        (y,), r = run(rt, backend, wt.type, [(wq, 512, 8, st, src, 9)], variant)
        assert r == name
        assert (np.abs(y.reshape(9, 8) - want) <= bound).all(), (name, np.abs(y.reshape(9, 8) - want).max())


@needs_ref
@ROWS
@pytest.mark.parametrize("K,N,B", SHAPES)
def test_reference_cpu(rt, backend, wt, K, N, B):
    m = [f32(W.weights(wt.type, K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)]
    for variant, name in both(wt):
        (y,), r = run(rt, backend, wt.type, m, variant)
        assert r == name
        assert W.rel_err(y, W._ref_mul_mat(wt.type, K, N, B)) <= W.TREE_TOL


@ROWS
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_one_fold(rt, backend, wt, K):
    N, B, T = 67, 68, wt.type
    ms = [f32(W.weights(T, K, N, 500 + i), K, N, synth.uniform(510 + i, K * B), B) for i in range(3)]
    alone = [run(rt, backend, T, [m], 16)[0][0] for m in ms]
    assert W.same_bits(run(rt, backend, T, [ms[0]], 128)[0][0], alone[0])  # the long shape against the short one
    for variant, name in both(wt):  # grouped in one graph against each alone
        ys, r = run(rt, backend, T, ms, variant)
        assert r == name and all(W.same_bits(y, a) for y, a in zip(ys, alone))
    wq, x = ms[0][0], ms[0][4]
    shards = [run(rt, backend, T, [f32(wq, K, N, x[c0 * K:c1 * K], c1 - c0)])[0][0] for c0, c1 in ((0, 32), (32, 68))]
    assert W.same_bits(np.concatenate(shards), alone[0])
