"""GGML_OP_FLASH_ATTN_EXT on MI355X against the reference CPU backend and against an f64 evaluation.

The same graph runs through the runtime + MI355X backend and through the reference library + its CPU
backend on the same bytes. The reference CPU rounds its V accumulator to f16 after every key and calls
libm's expf (src/ggml.c:15688-15733); the device accumulates in f32, so the two are not bit-identical
and every numeric test holds three bars, NMSE = sum((a - b)^2) / sum(b^2) over the non-NaN outputs:

  1. NMSE(device, reference CPU) <= 5e-4      the reference harness's own bar (test-backend-ops.cpp:1522)
  2. NMSE(device, f64 evaluation) <= 2^-22    an f32-accumulating kernel: at most one f16 rounding
                                              (2^-11 relative) per probability
  3. kv >= 64: NMSE(device, f64) <= NMSE(reference CPU, f64)

The f64 evaluation takes the same f16-rounded Q, K, V and mask. NaN positions (query rows all of whose
keys are masked: the reference's 0 / 0) must coincide exactly in all three.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
from ggml_mi355x import synth

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]

F32, F16, I32, Q4_K, Q8_0 = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32, G.GGML_TYPE_Q4_K, G.GGML_TYPE_Q8_0
PAD = G.GGML_KQ_MASK_PAD
HEAD_SIZES = (64, 80, 96, 112, 128, 256)
BAR_CPU = 5e-4
BAR_EXACT = 2.0 ** -22
NEG_INF = np.float16(-np.inf)


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


def pad_rows(n):
    return -(-n // PAD) * PAD


def run_graph(L, backend, build, n_tensors=96, computes=1, plan=False, extra=None):
    """build(L, ctx) -> (feeds, outs): outs is a list of (name, tensor), expanded into the graph in order.
    Returns name -> f32 array of the tensor's bytes (after `computes` computes, or plan replays)."""
    with G.Context(L, L.ggml_tensor_overhead() * n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
        feeds, outs = build(L, c.ctx)
        g = L.ggml_new_graph(c.ctx)
        for _, t in outs:
            L.ggml_build_forward_expand(g, t)
        buf = L.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            if plan:
                p = L.ggml_backend_graph_plan_create(backend, g)
                assert p
                for _ in range(computes):
                    assert L.ggml_backend_graph_plan_compute(backend, p) == G.GGML_STATUS_SUCCESS
                L.ggml_backend_synchronize(backend)
                L.ggml_backend_graph_plan_free(backend, p)
            else:
                for _ in range(computes):
                    assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            if extra is not None:
                extra(L, backend)
            return {name: G.tensor_get(L, t, np.float32) for name, t in outs}
        finally:
            L.ggml_backend_buffer_free(buf)


# ---- inputs and the f64 evaluation -------------------------------------------------------------------

def uniform(seed, *shape):
    return synth.uniform(seed, int(np.prod(shape))).reshape(shape).astype(np.float32)


def make_mask(kind, N, kv, seed):
    """[N, kv] f16, or None. causal: -inf above the diagonal of the last N keys."""
    if kind == "none":
        return None
    if kind == "rand":
        return uniform(seed, N, kv).astype(np.float16)
    assert kind == "causal"
    m = np.zeros((N, kv), np.float16)
    for i in range(N):
        m[i, max(kv - N + i + 1, 0):] = NEG_INF
    return m


def alibi_slopes(nh, max_bias):
    """src/ggml.c:15650-15664, in f32"""
    if max_bias <= 0.0:
        return np.ones(nh, np.float32)
    n2 = 1 << int(np.floor(np.log2(nh)))
    m0 = np.float32(2.0) ** np.float32(-max_bias / n2)
    m1 = np.float32(2.0) ** np.float32(-(max_bias / 2.0) / n2)
    return np.array([np.power(m0, np.float32(h + 1)) if h < n2 else np.power(m1, np.float32(2 * (h - n2) + 1))
                     for h in range(nh)], np.float32)


def exact_attention(q, k, v, mask, scale, max_bias):
    """q [ne3, nh, N, D] f32, k / v [ne3_kv, nh_kv, kv, D] f16, mask [N, kv] f16 or None -> [ne3, N, nh, D] f64"""
    ne3, nh, N, D = q.shape
    ne3k, nhk, kv, _ = k.shape
    ne3v, nhv = v.shape[:2]
    slopes = alibi_slopes(nh, max_bias)
    q16 = q.astype(np.float16).astype(np.float64)
    out = np.empty((ne3, N, nh, D), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i3 in range(ne3):
            for h in range(nh):
                K = k[i3 // (ne3 // ne3k), h // (nh // nhk)].astype(np.float64)
                V = v[i3 // (ne3 // ne3v), h // (nh // nhv)].astype(np.float64)
                s = q16[i3, h] @ K.T * np.float64(np.float32(scale))
                if mask is not None:
                    s = s + (slopes[h] * mask.astype(np.float32)).astype(np.float64)
                m = s.max(axis=1, keepdims=True)
                p = np.exp(s - m)
                out[i3, :, h, :] = (p @ V) / p.sum(axis=1, keepdims=True)
    return out


def nmse(a, b, keep):
    a, b = a[keep].astype(np.float64), b[keep].astype(np.float64)
    return float(np.sum((a - b) ** 2) / np.sum(b ** 2))


def check(dev, cpu, exact, kv, what):
    dev, cpu, exact = dev.reshape(-1), cpu.reshape(-1), exact.reshape(-1)
    nan = np.isnan(exact)
    assert np.array_equal(np.isnan(cpu), nan), f"{what}: the reference's NaN rows are not the f64 evaluation's"
    assert np.array_equal(np.isnan(dev), nan), f"{what}: NaN at {int(np.sum(np.isnan(dev) != nan))} wrong positions"
    keep = ~nan
    assert np.all(np.isfinite(dev[keep])), what
    e_cpu, e_dev, e_ref = nmse(dev, cpu, keep), nmse(dev, exact, keep), nmse(cpu, exact, keep)
    print(f"{what}: NMSE device/cpu {e_cpu:.2e}, device/f64 {e_dev:.2e}, cpu/f64 {e_ref:.2e}, NaN {int(nan.sum())}")
    assert e_cpu <= BAR_CPU, (what, e_cpu)
    assert e_dev <= BAR_EXACT, (what, e_dev)
    if kv >= 64:
        assert e_dev <= e_ref, (what, e_dev, e_ref)


class Case:
    """One plain-layout flash-attention node and its inputs."""

    def __init__(self, D, N, kv, nh=4, nh_kv=2, ne3=1, ne3_kv=1, mask="rand", max_bias=0.0, seed=1, prec=None):
        self.D, self.N, self.kv, self.nh, self.nh_kv, self.ne3, self.ne3_kv = D, N, kv, nh, nh_kv, ne3, ne3_kv
        self.max_bias, self.prec = max_bias, prec
        self.scale = float(1.0 / np.sqrt(D))
        self.q = uniform(seed, ne3, nh, N, D)
        self.k = uniform(seed + 1, ne3_kv, nh_kv, kv, D).astype(np.float16)
        self.v = uniform(seed + 2, ne3_kv, nh_kv, kv, D).astype(np.float16)
        self.mask = mask if isinstance(mask, np.ndarray) or mask is None else make_mask(mask, N, kv, seed + 3)
        self.what = f"D={D} N={N} kv={kv} nh={nh}/{nh_kv} ne3={ne3}/{ne3_kv} mask={mask if isinstance(mask, str) else 'given'} bias={max_bias}"

    def node(self, L, c, feeds):
        q = L.ggml_new_tensor_4d(c, F32, self.D, self.N, self.nh, self.ne3)
        k = L.ggml_new_tensor_4d(c, F16, self.D, self.kv, self.nh_kv, self.ne3_kv)
        v = L.ggml_new_tensor_4d(c, F16, self.D, self.kv, self.nh_kv, self.ne3_kv)
        feeds += [(q, self.q), (k, self.k), (v, self.v)]
        m = None
        if self.mask is not None:
            rows = pad_rows(self.N)
            m = L.ggml_new_tensor_2d(c, F16, self.kv, rows)
            full = np.full((rows, self.kv), np.nan, np.float16)  # the padding rows are never read
            full[:self.N] = self.mask
            feeds.append((m, full))
        r = L.ggml_flash_attn_ext(c, q, k, v, m, self.scale, self.max_bias)
        if self.prec is not None:
            L.ggml_flash_attn_ext_set_prec(r, self.prec)
        return r

    def build(self, L, c):
        feeds = []
        return feeds, [("out", self.node(L, c, feeds))]

    def exact(self):
        return exact_attention(self.q, self.k, self.v, self.mask, self.scale, self.max_bias)


def run_case(libs, case):
    rt, be, ref, cpu = libs
    dev = run_graph(rt, be, case.build)["out"]
    want = run_graph(ref, cpu, case.build)["out"]
    check(dev, want, case.exact(), case.kv, case.what)
    return dev


# ---- head sizes x row counts ---------------------------------------------------------------------------

FEW_ROWS = ((1, 1), (1, 33), (1, 257), (3, 64), (8, 1024))     # N * (nh / nh_kv) <= 16 rows per KV head
MANY_ROWS = ((9, 40), (33, 97), (70, 130))                      # ragged in N and kv, N across the mask padding


@pytest.mark.parametrize("N,kv", FEW_ROWS + MANY_ROWS)
@pytest.mark.parametrize("D", HEAD_SIZES)
def test_head_sizes_and_row_counts(libs, D, N, kv):
    for i, mask in enumerate(("none", "rand", "causal")):
        run_case(libs, Case(D, N, kv, mask=mask, seed=1000 + 10 * D + N + i))


@pytest.mark.parametrize("N", [31, 32])
@pytest.mark.parametrize("D", [80, 128, 256])
def test_kernel_threshold(libs, D, N):
    """Below 32 queries the register kernel runs (here in several row blocks), from 32 the MFMA kernel."""
    run_case(libs, Case(D, N, 100, nh=4, nh_kv=2, mask="causal", seed=300 + N))
    run_case(libs, Case(D, N, 64, nh=2, nh_kv=2, mask="rand", seed=310 + N))


# ---- heads ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nh_kv", [8, 2, 1])
@pytest.mark.parametrize("N", [1, 2, 20])
def test_grouped_query_heads(libs, nh_kv, N):
    run_case(libs, Case(128, N, 257, nh=8, nh_kv=nh_kv, mask="rand", seed=20 + nh_kv + N))


@pytest.mark.parametrize("nh_kv", [12, 4])
@pytest.mark.parametrize("N,kv", [(1, 200), (5, 97), (40, 130)])
def test_alibi_non_power_of_two_heads(libs, nh_kv, N, kv):
    """12 heads: heads 0..7 take m0^(h + 1), heads 8..11 take m1^(2 (h - 8) + 1)."""
    run_case(libs, Case(64, N, kv, nh=12, nh_kv=nh_kv, mask="rand", max_bias=8.0, seed=40 + N))
    run_case(libs, Case(80, N, kv, nh=12, nh_kv=nh_kv, mask="causal", max_bias=8.0, seed=50 + N))


@pytest.mark.parametrize("N,kv", [(2, 100), (33, 70)])
def test_batch_broadcast(libs, N, kv):
    """ne3 = 2 queries against ne3 = 1 K / V"""
    run_case(libs, Case(96, N, kv, nh=4, nh_kv=2, ne3=2, ne3_kv=1, mask="rand", seed=60 + N))
    run_case(libs, Case(128, N, kv, nh=4, nh_kv=4, ne3=2, ne3_kv=2, mask="none", seed=70 + N))


def test_precision_param(libs):
    """GGML_PREC_F32 and GGML_PREC_DEFAULT run the same kernels: the same bits"""
    rt, be, _, _ = libs
    a = run_case(libs, Case(128, 3, 300, mask="rand", seed=80, prec=G.GGML_PREC_F32))
    b = run_graph(rt, be, Case(128, 3, 300, mask="rand", seed=80, prec=G.GGML_PREC_DEFAULT).build)["out"]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the split rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kv,launches", [(100, 1), (128, 1), (129, 2), (4096, 2)])
def test_split_rule(libs, kv, launches):
    """Few rows over few KV heads: above 128 keys the KV range is split over workgroups and a combine
    kernel merges the partials (two launches); up to 128 keys one launch writes dst itself."""
    rt, be, ref, cpu = libs
    case = Case(128, 2, kv, nh=8, nh_kv=2, mask="causal", seed=90 + kv)
    n = []
    dev = run_graph(rt, be, case.build, extra=lambda L, b: n.append(L.ggml_backend_mi355x_last_launch_count(b)))["out"]
    assert n == [launches], n
    check(dev, run_graph(ref, cpu, case.build)["out"], case.exact(), kv, case.what)


# ---- llama.cpp's layout --------------------------------------------------------------------------------

@pytest.mark.parametrize("D,N,kv,row_pad", [(128, 1, 300, 0), (128, 4, 77, 0), (80, 40, 130, 0), (64, 33, 64, 0),
                                            (128, 3, 300, 4), (96, 40, 130, 4)])
def test_llama_cpp_layout(libs, D, N, kv, row_pad):
    """K and V are 3-D views of the first kv positions of a larger f16 cache whose unused positions hold
    NaN, Q is the permute(0, 2, 1, 3) of [D, nh, N], the mask is wider and taller than needed (the
    surplus holds NaN), and dst lies between sentinel tensors that must stay as they were. row_pad:
    extra halves per cache row (NaN), so that K / V rows start on 8-byte boundaries only and the
    kernels take their 2-byte loads."""
    nh, nh_kv, n_ctx = 8, 2, kv + 37
    scale = float(1.0 / np.sqrt(D))
    q = uniform(1, N, nh, D)                                        # [D, nh, N]
    cache = {}
    for name, seed in (("k", 2), ("v", 3)):
        a = np.full((n_ctx, nh_kv, D), np.nan, np.float16)          # [D * nh_kv (+ row_pad), n_ctx]
        a[:kv] = uniform(seed, kv, nh_kv, D).astype(np.float16)
        cache[name] = a
    padded = {name: np.concatenate([a.reshape(n_ctx, nh_kv * D), np.full((n_ctx, row_pad), np.nan, np.float16)], axis=1)
              for name, a in cache.items()}
    mask = make_mask("causal", N, kv, 0)
    mask[:, ::7] = NEG_INF                                          # some cells of other sequences
    mask[:, 0] = 0
    mcols, mrows = kv + 19, pad_rows(N) + PAD
    mfull = np.full((mrows, mcols), np.nan, np.float16)
    mfull[:N, :kv] = mask
    sent = {}

    def build(L, c):
        qt = L.ggml_new_tensor_3d(c, F32, D, nh, N)
        kc = L.ggml_new_tensor_2d(c, F16, D * nh_kv + row_pad, n_ctx)
        vc = L.ggml_new_tensor_2d(c, F16, D * nh_kv + row_pad, n_ctx)
        mt = L.ggml_new_tensor_2d(c, F16, mcols, mrows)
        row = kc.contents.nb[1]
        kview = L.ggml_view_3d(c, kc, D, kv, nh_kv, row, D * 2, 0)
        vview = L.ggml_view_3d(c, vc, D, kv, nh_kv, row, D * 2, 0)
        s1 = L.ggml_new_tensor_1d(c, F32, 1024)
        r = L.ggml_flash_attn_ext(c, L.ggml_permute(c, qt, 0, 2, 1, 3), kview, vview, mt, scale, 0.0)
        s2 = L.ggml_new_tensor_1d(c, F32, 1024)
        sent[L] = (s1, r, s2)
        pat = np.arange(1024, dtype=np.float32) + 0.5
        return [(qt, q), (kc, padded["k"]), (vc, padded["v"]), (mt, mfull), (s1, pat), (s2, -pat)], [("out", r)]

    rt, be, ref, cpu = libs
    kept = {}

    def sentinels(L, b):
        s1, r, s2 = sent[L]
        a1, ar, a2 = (int(t.contents.data) for t in (s1, r, s2))
        assert a1 + 4096 <= ar and ar + L.ggml_nbytes(r) <= a2 and a2 - (ar + L.ggml_nbytes(r)) < 1024 and ar - (a1 + 4096) < 1024
        kept["s1"], kept["s2"] = G.tensor_get(L, s1), G.tensor_get(L, s2)

    dev = run_graph(rt, be, build, extra=sentinels)["out"]
    pat = np.arange(1024, dtype=np.float32) + 0.5
    assert np.array_equal(kept["s1"], pat) and np.array_equal(kept["s2"], -pat), "dst's neighbours were written"
    want = run_graph(ref, cpu, build)["out"]
    k4 = cache["k"][:kv].transpose(1, 0, 2)[None]
    v4 = cache["v"][:kv].transpose(1, 0, 2)[None]
    exact = exact_attention(q.transpose(1, 0, 2)[None], k4, v4, mask, scale, 0.0)
    check(dev, want, exact, kv, f"llama.cpp layout D={D} N={N} kv={kv} row_pad={row_pad}")


# ---- -inf handling -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,kv", [(2, 300), (40, 300)])
@pytest.mark.parametrize("D", [64, 128])
def test_minus_infinity(libs, D, N, kv):
    """Keys masked at scattered positions (cells of other sequences), 64 consecutive keys masked in the
    middle for every query, and one query row all of whose keys are masked: NaN exactly there (the
    reference's 0 / 0) and nowhere else."""
    rng = np.random.default_rng(7 + N)
    mask = uniform(5, N, kv).astype(np.float16)
    mask[rng.random((N, kv)) < 0.3] = NEG_INF
    mask[:, 64:128] = NEG_INF
    mask[:, 200] = 0
    mask[N // 2, :] = NEG_INF
    dev = run_case(libs, Case(D, N, kv, nh=4, nh_kv=2, mask=mask, seed=100 + N))
    out = dev.reshape(N, 4, D)
    assert np.all(np.isnan(out[N // 2])) and int(np.isnan(out).sum()) == 4 * D


# ---- determinism ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,kv", [(1, 2000), (8, 300), (40, 130)])
def test_repeatable_and_plan_replay(libs, N, kv):
    """Two computes give the same bits, and a graph plan replayed twice gives the bits of the direct
    compute (with a split KV range too: the combine adds the partials in index order)."""
    rt, be, _, _ = libs
    case = Case(128, N, kv, nh=8, nh_kv=2, mask="causal", seed=110 + N)
    a = run_graph(rt, be, case.build)["out"].view(np.uint32)
    b = run_graph(rt, be, case.build, computes=2)["out"].view(np.uint32)
    p = run_graph(rt, be, case.build, computes=2, plan=True)["out"].view(np.uint32)
    assert np.array_equal(a, b)
    assert np.array_equal(a, p)


def test_two_nodes_in_one_graph(libs):
    """Two flash-attention nodes of different shapes, both with a split KV range, in one graph: each
    equals its single-node result bit for bit (no shared partials)."""
    rt, be, _, _ = libs
    c1 = Case(128, 1, 3000, nh=8, nh_kv=2, mask="rand", seed=120)
    c2 = Case(64, 3, 1500, nh=4, nh_kv=1, mask="causal", seed=130)

    def build(L, c):
        feeds = []
        return feeds, [("a", c1.node(L, c, feeds)), ("b", c2.node(L, c, feeds))]

    for plan in (False, True):
        both = run_graph(rt, be, build, plan=plan, computes=2 if plan else 1)
        assert np.array_equal(both["a"].view(np.uint32), run_graph(rt, be, c1.build)["out"].view(np.uint32))
        assert np.array_equal(both["b"].view(np.uint32), run_graph(rt, be, c2.build)["out"].view(np.uint32))


# ---- a LLaMA-shaped block with flash attention -------------------------------------------------------------

E, H, H_KV, FF, N_PAST, N_CTX = 512, 8, 2, 1536, 3, 64
HD = E // H
E_KV = HD * H_KV


def _block_weights(wtype):
    rt = G.runtime()
    w = {}
    for i, (name, k, n) in enumerate((("wq", E, E), ("wk", E, E_KV), ("wv", E, E_KV), ("wo", E, E), ("w1", E, FF), ("w3", E, FF),
                                      ("w2", FF, E))):
        f = (synth.uniform(100 + i, k * n) * np.float32(0.08)).astype(np.float32)
        if wtype == F16:
            w[name] = (f.astype(np.float16), k, n)
        else:
            out = np.empty(G.row_size(wtype, k) * n, np.uint8)
            rt.ggml_quantize_chunk(wtype, f.ctypes.data, out.ctypes.data, 0, n, k, None)
            w[name] = (out, k, n)
    w["attn_norm"] = (1.0 + 0.1 * synth.uniform(120, E)).astype(np.float32)
    w["ffn_norm"] = (1.0 + 0.1 * synth.uniform(121, E)).astype(np.float32)
    return w


def _build_block(L, c, W, wtype, T, x):
    """llama.cpp's build_llama with flash attention: K / V of the new tokens are written into an f16
    cache by ggml_cpy, attention reads views of the cache's first N_PAST + T positions."""
    feeds = []

    def new(t, arr, *ne):
        tt = {1: L.ggml_new_tensor_1d, 2: L.ggml_new_tensor_2d}[len(ne)](c, t, *ne)
        feeds.append((tt, arr))
        return tt

    kv = N_PAST + T
    xt = new(F32, x, E, T)
    pt = new(I32, (np.arange(T, dtype=np.int32) + N_PAST).astype(np.int32), T)
    wt = {k: new(wtype, v[0], v[1], v[2]) for k, v in W.items() if k.startswith("w")}
    an = new(F32, W["attn_norm"], E)
    fn_ = new(F32, W["ffn_norm"], E)
    caches = []
    for seed in (140, 141):
        a = np.full((N_CTX, E_KV), np.nan, np.float16)
        a[:N_PAST] = (uniform(seed, N_PAST, E_KV) * np.float32(0.5)).astype(np.float16)
        caches.append(new(F16, a, E_KV, N_CTX))
    kc, vc = caches
    mask = np.full((pad_rows(T), kv), np.nan, np.float16)
    mask[:T] = 0
    for i in range(T):
        mask[i, N_PAST + i + 1:] = NEG_INF
    mt = new(F16, mask, kv, pad_rows(T))

    h = L.ggml_mul(c, L.ggml_rms_norm(c, xt, 1e-5), an)
    q = L.ggml_rope(c, L.ggml_reshape_3d(c, L.ggml_mul_mat(c, wt["wq"], h), HD, H, T), pt, HD, 0, 0)
    k = L.ggml_rope(c, L.ggml_reshape_3d(c, L.ggml_mul_mat(c, wt["wk"], h), HD, H_KV, T), pt, HD, 0, 0)
    v = L.ggml_mul_mat(c, wt["wv"], h)
    row = kc.contents.nb[1]
    k_cpy = L.ggml_cpy(c, L.ggml_reshape_2d(c, k, E_KV, T), L.ggml_view_2d(c, kc, E_KV, T, row, N_PAST * row))
    v_cpy = L.ggml_cpy(c, v, L.ggml_view_2d(c, vc, E_KV, T, row, N_PAST * row))
    K = L.ggml_view_3d(c, kc, HD, kv, H_KV, row, HD * 2, 0)
    V = L.ggml_view_3d(c, vc, HD, kv, H_KV, row, HD * 2, 0)
    att = L.ggml_flash_attn_ext(c, L.ggml_permute(c, q, 0, 2, 1, 3), K, V, mt, float(1.0 / np.sqrt(HD)), 0.0)
    cur = L.ggml_reshape_2d(c, att, E, T)
    out = L.ggml_add(c, L.ggml_mul_mat(c, wt["wo"], cur), xt)
    h2 = L.ggml_mul(c, L.ggml_rms_norm(c, out, 1e-5), fn_)
    g = L.ggml_mul_mat(c, wt["w1"], h2)
    u = L.ggml_mul_mat(c, wt["w3"], h2)
    y = L.ggml_add(c, L.ggml_mul_mat(c, wt["w2"], L.ggml_mul(c, L.ggml_silu(c, g), u)), out)
    # the cache writes go into the graph ahead of their reader, as llama.cpp expands them
    return feeds, [("k_cpy", k_cpy), ("v_cpy", v_cpy), ("att", att), ("out", y)]


@pytest.mark.parametrize("T", [1, 40])
@pytest.mark.parametrize("wtype", [Q4_K, F16], ids=["q4_K", "f16"])
def test_llama_block_with_flash_attention(libs, wtype, T):
    """The block of tests/test_llama_block_gpu.py with GGML_OP_FLASH_ATTN_EXT in place of its KQ /
    soft_max / KQV chain, GQA 4:1 and an f16 K/V cache written by ggml_cpy in the same graph. The f64
    truth of a quantized block is not defined here: the block output is held to the harness's NMSE
    5e-4 against the reference CPU on the same graph."""
    rt, be, ref, cpu = libs
    W = _block_weights(wtype)
    x = (synth.uniform(7, E * T) * np.float32(2.0)).astype(np.float32)
    a = run_graph(rt, be, lambda L, c: _build_block(L, c, W, wtype, T, x), n_tensors=128)
    b = run_graph(ref, cpu, lambda L, c: _build_block(L, c, W, wtype, T, x), n_tensors=128)
    for name in ("att", "out"):
        assert np.all(np.isfinite(b[name])) and np.all(np.isfinite(a[name])), name
        e = nmse(a[name], b[name], np.ones(a[name].shape, bool))
        print(f"{'f16' if wtype == F16 else 'q4_K'} block T={T} {name}: NMSE {e:.2e}")
        assert e <= BAR_CPU, (name, e)


# ---- supports_op ---------------------------------------------------------------------------------------

def test_supports_op(libs):
    """Asked, never computed."""
    rt, be, _, _ = libs
    with G.Context(rt, rt.ggml_tensor_overhead() * 256, no_alloc=True) as cx:
        c = cx.ctx
        sup = lambda t: bool(rt.ggml_backend_supports_op(be, t))

        def fa(D=128, N=4, kv=96, nh=8, nh_kv=2, ktype=F16, vtype=F16, mask=True, max_bias=0.0):
            q = rt.ggml_new_tensor_4d(c, F32, D, N, nh, 1)
            k = rt.ggml_new_tensor_4d(c, ktype, D, kv, nh_kv, 1)
            v = rt.ggml_new_tensor_4d(c, vtype, D, kv, nh_kv, 1)
            m = rt.ggml_new_tensor_2d(c, F16, kv, pad_rows(N)) if mask else None
            return rt.ggml_flash_attn_ext(c, q, k, v, m, 0.1, max_bias), (q, k, v, m)

        for D in HEAD_SIZES:
            for mask in (True, False):
                assert sup(fa(D=D, mask=mask)[0]), D
        assert sup(fa(max_bias=8.0)[0])
        assert sup(fa(nh=12, nh_kv=4, max_bias=8.0)[0])
        assert not sup(fa(D=72)[0])
        assert not sup(fa(D=32)[0])
        assert not sup(fa(ktype=F32, vtype=F32)[0])
        assert not sup(fa(D=128, ktype=Q8_0, vtype=Q8_0)[0])
        assert not sup(fa(vtype=F32)[0])
        # ALiBi without a mask: the builder refuses it, so the node is altered after it was built
        r, _ = fa(mask=False)
        r.contents.op_params[1] = np.float32(8.0).view(np.int32).item()
        assert not sup(r)
        # a mask that is not contiguous (a view of the first 96 columns of wider rows), F32 mask
        r, (q, k, v, m) = fa()
        wide = rt.ggml_new_tensor_2d(c, F16, 128, 32)
        view = rt.ggml_view_2d(c, wide, 96, 32, wide.contents.nb[1], 0)
        r.contents.src[3] = ctypes.cast(view, ctypes.c_void_p).value
        assert not sup(r)
        r.contents.src[3] = ctypes.cast(rt.ggml_new_tensor_2d(c, F32, 96, 32), ctypes.c_void_p).value
        assert not sup(r)
        # a mask with fewer columns than keys
        r.contents.src[3] = ctypes.cast(rt.ggml_new_tensor_2d(c, F16, 64, 32), ctypes.c_void_p).value
        assert not sup(r)
        # K in a split buffer
        split = rt.ggml_backend_mi355x_split_buffer_type(None)
        with G.Context(rt, rt.ggml_tensor_overhead() * 8, no_alloc=True) as cs:
            ks = rt.ggml_new_tensor_2d(cs.ctx, F16, 128, 96)
            buf = rt.ggml_backend_alloc_ctx_tensors_from_buft(cs.ctx, split)
            assert buf
            try:
                r, _ = fa(nh=8, nh_kv=1)
                r.contents.src[1] = ctypes.cast(ks, ctypes.c_void_p).value
                assert not sup(r)
            finally:
                rt.ggml_backend_buffer_free(buf)
