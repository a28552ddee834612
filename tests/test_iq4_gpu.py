"""GPU tests of IQ4_NL and IQ4_XS weights on the MI355X backend: GET_ROWS, MUL_MAT and MUL_MAT_ID in the
reference CPU's summation order (mmv_order=1: identical bits) and in tree order (mmv_order=0: within
1e-5 of the largest reference value), the default order of a quantized graph, a tiny GPT-2 of each
type end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/iq4nl_*, iq4xs_*
where those suffice. All the assertions are path-agnostic: they hold whichever kernel serves a shape.
"""
import ctypes
import functools
import json
import os

os.environ.setdefault("GGML_MI355X_SPLIT_SLOTS", "3")  # read once, at the first split buffer type (as tests/test_split_gpu.py)

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import gguf
from ggml_mi355x import gpt2
from ggml_mi355x import synth

pytestmark = pytest.mark.gpu

REF = os.path.join(REPO, "oracle", "_ref")
REF_LIB = os.path.join(REF, "libggml_ref.so")
REF_GPT2 = os.path.join(REF, "libgpt2_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference lib not built (make -C oracle ref)")
IQ4_NL, IQ4_XS, Q8_0, Q8_K = 20, 23, 8, 15
TAG = {IQ4_NL: "iq4nl", IQ4_XS: "iq4xs"}
FTYPE = {IQ4_NL: "iq4_nl", IQ4_XS: "iq4_xs"}
ACT = {IQ4_NL: Q8_0, IQ4_XS: Q8_K}  # the vec_dot_type
both_types = pytest.mark.parametrize("T", [IQ4_NL, IQ4_XS], ids=lambda t: TAG[t])
TREE_TOL = 1e-5  # integer block sums are exact: only the f32 combination order differs

with open(os.path.join(GOLDEN, "iq4.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def backend(rt):
    b = G.mi355x_backend(rt, 0)
    yield b
    rt.ggml_backend_free(b)


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


def rel_err(y, r):
    return float(np.abs(y.astype(np.float64) - r).max() / max(np.abs(r).max(), 1e-30))


def same_bits(y, r):
    return np.array_equal(y.view(np.uint32), r.view(np.uint32))


def in_order(rt, order, fn):
    assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
    try:
        return fn()
    finally:
        rt.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)


@functools.lru_cache(maxsize=None)
def weights(T, K, N, seed):
    """Seeded rows of type T from the runtime's quantizer (tests/test_iq4.py pins it to the reference's bytes)."""
    rt = G.runtime()
    w = np.random.default_rng(seed).standard_normal(K * N).astype(np.float32)
    out = np.empty(G.row_size(T, K) * N, np.uint8)
    assert rt.ggml_quantize_chunk(T, w.ctypes.data, out.ctypes.data, 0, N, K, None) == out.nbytes
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ GET_ROWS

@both_types
@pytest.mark.parametrize("which", ["w", "edge"])
def test_get_rows_matches_golden_dequantization(rt, backend, T, which):
    """Row indices out of order and repeated, f32 dst: dequantize_row_iq4_nl's / _iq4_xs's bits, the
    -0.0 elements of IQ4_XS's all-zero superblock (edge row 0) included."""
    K, N = MANIFEST[which]["K"], MANIFEST[which]["N"]
    wq = golden_blob(f"{TAG[T]}_{which}.wq.bin")
    want = golden_blob(f"{TAG[T]}_{which}.wdq.f32", np.float32).reshape(N, K)
    idx = np.array([N - 1, 0, 2, 2, 1, N - 1, 3, 0, N - 2], np.int32)
    if which == "edge" and T == IQ4_XS:
        assert (want[0, :256].view(np.uint32) == 0x80000000).all()  # the fixture does hold the -0.0 superblock

    def build(c):
        w = rt.ggml_new_tensor_2d(c, T, K, N)
        i = rt.ggml_new_tensor_1d(c, G.GGML_TYPE_I32, len(idx))
        return [(w, wq), (i, idx)], rt.ggml_get_rows(c, w, i)

    y = G.graph_once(rt, backend, build).reshape(len(idx), K)
    assert same_bits(y, want[idx]), float(np.abs(y - want[idx]).max())


# ------------------------------------------------------------------ MUL_MAT

@both_types
def test_mul_mat_matches_golden_output(rt, backend, T):
    """The committed reference-CPU output (B = 3): identical bits in order 1, 1e-5 in tree order."""
    c = MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wq = golden_blob(f"{TAG[T]}_w.wq.bin")
    x = synth.uniform(c["xseed"], K * B)
    want = golden_blob(f"{TAG[T]}_w.y.f32", np.float32)
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
    print(f"golden {TAG[T]} B={B}: order 1 rel err {rel_err(y1, want):.2e}, tree order {rel_err(y0, want):.2e}")
    assert same_bits(y1, want), rel_err(y1, want)
    assert rel_err(y0, want) <= TREE_TOL


# one superblock; one item per lane of a wave (K 4096: IQ4_NL two); 43 superblocks, 5848-byte IQ4_XS
# rows (8 mod 16) and more than two items per lane (K 11008); N not a multiple of the rows per
# workgroup. IQ4_NL also rows that are no multiple of 256 (an even block count: 2 and 10 blocks), which
# only the generic kernels take. 1..8 columns in one launch, 8-column chunks with a tail of 1, and two
# whole chunks.
SHAPES = {IQ4_NL: [(256, 33), (4096, 64), (11008, 16), (64, 16), (320, 40)], IQ4_XS: [(256, 33), (4096, 64), (11008, 16)]}
CASES = [(T, K, N) for T in (IQ4_NL, IQ4_XS) for K, N in SHAPES[T]]
CASE_IDS = [f"{TAG[T]}-{K}x{N}" for T, K, N in CASES]
COLS = [1, 2, 5, 8, 9, 16]


@functools.lru_cache(maxsize=None)
def _ref_mul_mat(T, K, N, B):
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    try:
        y = G.mul_mat_once(lib, cpu, T, weights(T, K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)
    finally:
        lib.ggml_backend_free(cpu)
    y.setflags(write=False)
    return y


@needs_ref
@pytest.mark.parametrize("T,K,N", CASES, ids=CASE_IDS)
def test_mul_mat_reference_order_bit_identical(rt, backend, T, K, N):
    wq = weights(T, K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        yr = _ref_mul_mat(T, K, N, B)
        assert same_bits(y, yr), (B, float(np.mean(y.view(np.uint32) == yr.view(np.uint32))), rel_err(y, yr))


@needs_ref
@pytest.mark.parametrize("T,K,N", CASES, ids=CASE_IDS)
def test_mul_mat_tree_order(rt, backend, T, K, N):
    wq = weights(T, K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        err = rel_err(y, _ref_mul_mat(T, K, N, B))
        print(f"tree order {TAG[T]} K={K} N={N} B={B}: rel err {err:.2e}")
        assert err <= TREE_TOL, (B, err)


@needs_ref
@both_types
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref, T):
    """LLaMA-7B's ffn_down row shape, 11008 -> 64: 43 superblocks, IQ4_XS rows of 5848 bytes (every
    other row starts 8 mod 16), 344 IQ4_NL / 172 IQ4_XS items per row. Decode and prompt column counts."""
    lib, cpu = ref
    K, N = 11008, 64
    wq = weights(T, K, N, 801)
    for B in (1, 3, 8, 9):
        x = synth.uniform(802 + B, K * B)
        yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yr), (B, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (B, rel_err(y0, yr))


def _mul_mat_general(lib, backend, T, wq, w_ne, x, x_ne, permute_x):
    """W [K, N, ne02, 1] x X [K, ne11, ne12, 1] with broadcasting; permute_x: X stored as
    [K, ne12, ne11] and permuted, so that src1's columns are strided."""
    ovh = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, ovh, no_alloc=True) as c:
        w = lib.ggml_new_tensor_4d(c.ctx, T, *w_ne)
        if permute_x:
            xs = lib.ggml_new_tensor_4d(c.ctx, G.GGML_TYPE_F32, x_ne[0], x_ne[2], x_ne[1], x_ne[3])
            xt = lib.ggml_permute(c.ctx, xs, 0, 2, 1, 3)
        else:
            xs = xt = lib.ggml_new_tensor_4d(c.ctx, G.GGML_TYPE_F32, *x_ne)
        y = lib.ggml_mul_mat(c.ctx, w, xt)
        g = lib.ggml_new_graph(c.ctx)
        lib.ggml_build_forward_expand(g, y)
        buf = lib.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        try:
            G.tensor_set(lib, w, wq)
            G.tensor_set(lib, xs, x)
            assert lib.ggml_backend_graph_compute(backend, g) == 0
            return G.tensor_get(lib, y)
        finally:
            lib.ggml_backend_buffer_free(buf)


@needs_ref
@both_types
@pytest.mark.parametrize("ne11", [1, 3, 9])
def test_weight_batch_and_strided_src1(rt, backend, ref, T, ne11):
    """A 3-D weight batch (ne02 = 2) broadcast over ne12 = 4, contiguous and strided src1."""
    lib, cpu = ref
    K, N, ne02, ne12 = 768, 40, 2, 4  # three superblocks: IQ4_XS rows 8 mod 16
    w_ne, x_ne = (K, N, ne02, 1), (K, ne11, ne12, 1)
    wq = weights(T, K, N * ne02, 301)
    x = synth.uniform(302 + ne11, K * ne11 * ne12)
    for permute in (False, True):
        yr = _mul_mat_general(lib, cpu, T, wq, w_ne, x, x_ne, permute)
        y1 = in_order(rt, 1, lambda: _mul_mat_general(rt, backend, T, wq, w_ne, x, x_ne, permute))
        y0 = in_order(rt, 0, lambda: _mul_mat_general(rt, backend, T, wq, w_ne, x, x_ne, permute))
        assert same_bits(y1, yr), (permute, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (permute, rel_err(y0, yr))


def _cpy_q8_then_mul_mat(lib, backend, T, wq, K, N, x, B):
    """X (f32) -> CPY to Q8_0 / Q8_K rows -> MUL_MAT(W, Xq) as one graph: src1 already of the vec_dot type."""
    overhead = lib.ggml_tensor_overhead() * 8 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        w = lib.ggml_new_tensor_2d(c.ctx, T, K, N)
        xt = lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, B)
        xq = lib.ggml_cpy(c.ctx, xt, lib.ggml_new_tensor_2d(c.ctx, ACT[T], K, B))
        y = lib.ggml_mul_mat(c.ctx, w, xq)
        g = lib.ggml_new_graph(c.ctx)
        lib.ggml_build_forward_expand(g, y)
        buf = lib.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf
        try:
            G.tensor_set(lib, w, wq)
            G.tensor_set(lib, xt, x)
            assert lib.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return G.tensor_get(lib, y)
        finally:
            lib.ggml_backend_buffer_free(buf)


@needs_ref
@both_types
@pytest.mark.parametrize("B", [1, 4])
def test_prequantized_src1(rt, backend, ref, T, B):
    """src1 already Q8_0 (IQ4_NL) / Q8_K (IQ4_XS) rows."""
    lib, cpu = ref
    K, N = 1024, 48
    wq = weights(T, K, N, 401)
    x = synth.uniform(402 + B, K * B)
    yr = _cpy_q8_then_mul_mat(lib, cpu, T, wq, K, N, x, B)
    y1 = in_order(rt, 1, lambda: _cpy_q8_then_mul_mat(rt, backend, T, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: _cpy_q8_then_mul_mat(rt, backend, T, wq, K, N, x, B))
    yf = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
    assert same_bits(y1, yf), rel_err(y1, yf)  # the same quants either way: the F32-src1 path's bits


def _three_mul_mats(lib, backend, T, wqs, K, N, xs):
    """Three independent same-shape mul_mats (B = 1) in one graph."""
    overhead = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        ws = [lib.ggml_new_tensor_2d(c.ctx, T, K, N) for _ in wqs]
        xts = [lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, 1) for _ in xs]
        ys = [lib.ggml_mul_mat(c.ctx, w, x) for w, x in zip(ws, xts)]
        g = lib.ggml_new_graph(c.ctx)
        for y in ys:
            lib.ggml_build_forward_expand(g, y)
        buf = lib.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf
        try:
            for t, a in list(zip(ws, wqs)) + list(zip(xts, xs)):
                G.tensor_set(lib, t, a)
            assert lib.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return [G.tensor_get(lib, y) for y in ys]
        finally:
            lib.ggml_backend_buffer_free(buf)


@needs_ref
@both_types
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref, T):
    lib, cpu = ref
    K, N = 4096, 64
    wqs = [weights(T, K, N, 500 + i) for i in range(3)]
    xs = [synth.uniform(510 + i, K) for i in range(3)]
    yr = _three_mul_mats(lib, cpu, T, wqs, K, N, xs)
    y1 = in_order(rt, 1, lambda: _three_mul_mats(rt, backend, T, wqs, K, N, xs))
    y0 = in_order(rt, 0, lambda: _three_mul_mats(rt, backend, T, wqs, K, N, xs))
    for i in range(3):
        assert same_bits(y1[i], yr[i]), (i, rel_err(y1[i], yr[i]))
        assert rel_err(y0[i], yr[i]) <= TREE_TOL, (i, rel_err(y0[i], yr[i]))


def _blocks(T, fill, d=1.0):
    """256 elements whose quant and scale bytes are all `fill`: 0x00 every code 0 (the level -127) and,
    IQ4_XS, every ls = 0 (the scale -32); 0xFF every code 15 (113) and every ls = 63 (31)."""
    dh = np.array([d], np.float16).view(np.uint8)
    if T == IQ4_NL:
        b = np.full((8, 18), fill, np.uint8)
        b[:, 0:2] = dh
    else:
        b = np.full((1, 136), fill, np.uint8)
        b[:, 0:2] = dh
    return b.ravel()


# columns whose quantized activations are all of the largest magnitude: constant columns (every
# quant 127 or -127 in Q8_0, -127 in Q8_K), alternating signs (+-127), and a small constant
EXTREME_X = (lambda K: np.concatenate([np.full(K, 0.5, np.float32), np.full(K, -2.0, np.float32)]),
             lambda K: np.concatenate([np.tile(np.array([3.0, -3.0], np.float32), K // 2), np.full(K, 1e-3, np.float32)]))


@needs_ref
@both_types
def test_extreme_integers(rt, backend, ref, T):
    """Hand-made blocks at the ends of the integer range against columns that quantize to +-127
    throughout (through an F32 src1 and through src1 pre-quantized by CPY alike). IQ4_XS with every
    code 0 (-127) and every scale -32 against -127 reaches the lane sum 8 * 4 * 127 * 127 * 32 =
    16 516 096 < 2^24; IQ4_NL the lane sum 4 * 127 * 127 per block. Identical bits in the reference
    order. K = 512, N = 8, B = 2."""
    lib, cpu = ref
    lo, hi = _blocks(T, 0x00), _blocks(T, 0xFF)
    pairs = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    wq = np.concatenate([np.concatenate(p) for p in pairs + pairs[::-1]])
    K, N, B = 512, 8, 2
    assert wq.size == N * G.row_size(T, K)
    for mk in EXTREME_X:
        x = mk(K)
        yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x, B)
        assert np.abs(yr).max() > 1.0  # the sums did not cancel
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yr), (y1, yr)
        assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
        yq = _cpy_q8_then_mul_mat(lib, cpu, T, wq, K, N, x, B)
        yq1 = in_order(rt, 1, lambda: _cpy_q8_then_mul_mat(rt, backend, T, wq, K, N, x, B))
        assert same_bits(yq1, yq), (yq1, yq)


@needs_ref
@both_types
def test_all_codes_rows_against_extreme_activations(rt, backend, ref, T):
    """The edge fixture (its last row holds all sixteen codes in both nibble halves of every block)
    against the +-127 columns: pins the codebook lookup entry by entry, in both orders."""
    lib, cpu = ref
    K, N, B = MANIFEST["edge"]["K"], MANIFEST["edge"]["N"], 2
    wq = golden_blob(f"{TAG[T]}_edge.wq.bin")
    for mk in EXTREME_X:
        x = mk(K)
        yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yr), (y1, yr)
        assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
    # one code at a time: a column that is 1 at element e alone picks the level of element e
    x = np.zeros((32, K), np.float32)
    x[np.arange(32), np.arange(32)] = 1.0
    yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x.ravel(), 32)
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x.ravel(), 32))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x.ravel(), 32))
    assert same_bits(y1, yr), (y1.reshape(32, N)[:, N - 1], yr.reshape(32, N)[:, N - 1])
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


@needs_ref
@both_types
@pytest.mark.parametrize("B", [1, 8])
def test_default_order_of_a_quantized_chain(rt, backend, ref, T, B):
    """W1 . x -> RMSNorm -> W2 with the default settings (mmv_order -1): the second mul_mat consumes
    computed activations, so the graph runs in the reference order -- the reference CPU's bits."""
    lib, cpu = ref
    K, N1, N2 = 1024, 768, 37
    w1, w2 = weights(T, K, N1, 601), weights(T, N1, N2, 602)
    x = synth.uniform(603 + B, K * B)

    def build(L, c):
        a = L.ggml_new_tensor_2d(c, T, K, N1)
        b = L.ggml_new_tensor_2d(c, T, N1, N2)
        xt = L.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, B)
        h = L.ggml_rms_norm(c, L.ggml_mul_mat(c, a, xt), 1e-5)
        return [(a, w1), (b, w2), (xt, x)], L.ggml_mul_mat(c, b, h)

    y = G.graph_once(rt, backend, lambda c: build(rt, c))
    yr = G.graph_once(lib, cpu, lambda c: build(lib, c))
    assert same_bits(y, yr), rel_err(y, yr)


@both_types
def test_supports_op_follows_the_table(rt, backend, T):
    """MUL_MAT, MUL_MAT_ID and GET_ROWS are taken; an IQ4_NL row of an odd block count is refused
    (the reference's AVX2 dot walks the blocks in pairs and defines no result there)."""
    def supported(K):
        with G.Context(rt, rt.ggml_tensor_overhead() * 8, no_alloc=True) as c:
            w = rt.ggml_new_tensor_2d(c.ctx, T, K, 4)
            x = rt.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, 2)
            i = rt.ggml_new_tensor_1d(c.ctx, G.GGML_TYPE_I32, 3)
            return (bool(rt.ggml_backend_supports_op(backend, rt.ggml_mul_mat(c.ctx, w, x))),
                    bool(rt.ggml_backend_supports_op(backend, rt.ggml_get_rows(c.ctx, w, i))))
    assert supported(256) == (True, True)
    if T == IQ4_NL:
        assert supported(64) == (True, True) and supported(320) == (True, True)
        assert supported(32) == (False, True) and supported(96) == (False, True)


# ------------------------------------------------------------------ MUL_MAT_ID

def _mul_mat_id(L, be, T, w, K, n, n_as, n_ids, n_tokens, x, ids):
    def build(c):
        a = L.ggml_new_tensor_3d(c, T, K, n, n_as)
        b = L.ggml_new_tensor_3d(c, G.GGML_TYPE_F32, K, 1, n_tokens)
        full = L.ggml_new_tensor_2d(c, G.GGML_TYPE_I32, n_as, n_tokens)
        top = L.ggml_view_2d(c, full, n_ids, n_tokens, full.contents.nb[1], 0)
        return [(a, w), (b, x), (full, ids)], L.ggml_mul_mat_id(c, a, b, top)
    return G.graph_once(L, be, build)


@needs_ref
@both_types
@pytest.mark.parametrize("n_tokens", [1, 5])
def test_mul_mat_id_top2_of_4_experts(rt, backend, ref, T, n_tokens):
    """4 experts, the first two ids of every token's row (a strided view), src1 broadcast over the
    ids: decode and a 5-token prompt against the reference CPU's MUL_MAT_ID."""
    lib, cpu = ref
    K, n, n_as, n_ids = 768, 100, 4, 2
    w = weights(T, K, n * n_as, 901)
    x = synth.uniform(902 + n_tokens, K * n_tokens)
    rng = np.random.default_rng(903 + n_tokens)
    ids = np.stack([rng.permutation(n_as) for _ in range(n_tokens)]).astype(np.int32)
    yr = _mul_mat_id(lib, cpu, T, w, K, n, n_as, n_ids, n_tokens, x, ids)
    y1 = in_order(rt, 1, lambda: _mul_mat_id(rt, backend, T, w, K, n, n_as, n_ids, n_tokens, x, ids))
    y0 = in_order(rt, 0, lambda: _mul_mat_id(rt, backend, T, w, K, n, n_as, n_ids, n_tokens, x, ids))
    assert yr.shape == (n * n_ids * n_tokens,) and np.abs(yr).max() > 0
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


# ------------------------------------------------------------------ GPT-2 end to end

TINY = dict(n_embd=256, n_head=4, n_layer=2, n_vocab=512, n_ctx=64)


@pytest.fixture(scope="module")
def tiny_models(tmp_path_factory):
    d = tmp_path_factory.mktemp("iq4_gpt2")
    f16 = gpt2.write_synthetic_model(str(d / "tiny-f16.bin"), **TINY)
    return f16, {T: gpt2.quantize_model(G.runtime(), f16, str(d / f"tiny-{FTYPE[T]}.bin"), FTYPE[T]) for T in (IQ4_NL, IQ4_XS)}


def _both_models(path, n_batch):
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, path, be, n_batch=n_batch)
    ref = G.Lib([REF_LIB, REF_GPT2], isolated=True)
    rbe = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(rbe, 4)
    rm = gpt2.Model(ref, path, rbe, n_batch=n_batch)

    def free():
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)
    return ours, rm, free


TOKENS = [(37 * i * i + 11 * i + 5) % 511 for i in range(20)]


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@both_types
@pytest.mark.parametrize("mode", ["decode", "prompt12"])
def test_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, T, mode):
    """A tiny GPT-2 of the type from quantize_model (model file ftype 19 / 22; its get_rows embedding,
    its MUL_MAT for every projection and the lm_head), default settings: teacher-forced decode over 8
    tokens and a 12-token prompt in one batch (the chunked > 8 column path) -- the reference CPU's
    logits on the same file, bit for bit."""
    n_batch = 12 if mode == "prompt12" else 8
    ours, rm, free = _both_models(tiny_models[1][T], n_batch)
    try:
        assert ours.hp.ftype % 1000 == gpt2.FTYPES[FTYPE[T]][0]
        steps = [[t] for t in TOKENS[:8]] if mode == "decode" else [TOKENS[:12]]
        n_past = 0
        for chunk in steps:
            a = ours.eval(n_past, chunk, all_logits=True)
            b = rm.eval(n_past, chunk, all_logits=True)
            assert np.isfinite(b).all() and np.abs(b).max() > 0
            assert same_bits(a, b), (mode, n_past, float(np.mean(a == b)), rel_err(a, b))
            n_past += len(chunk)
    finally:
        free()


# ------------------------------------------------------------------ split buffers, GGUF

def _split_buft(rt, props):
    arr = (ctypes.c_float * 16)(*([float(p) for p in props] + [0.0] * (16 - len(props))))
    return rt.ggml_backend_mi355x_split_buffer_type(ctypes.cast(arr, ctypes.c_void_p))


@both_types
@pytest.mark.parametrize("B", [1, 16])
def test_split_buffer_weights(rt, backend, T, B):
    """Rows divided over the slots of a split buffer (slots beyond the device count are virtual
    slots on device 0, each with its own allocation, stream and copies): each slice runs through the
    same mul_mat as the unsplit weight: the unsplit result's bits in the reference order, within
    1e-5 of it in tree order."""
    K, N = 768, 333  # 408-byte IQ4_XS rows: 8 mod 16
    wq = weights(T, K, N, 701)
    x = synth.uniform(702 + B, K * B)
    buft = _split_buft(rt, [1, 1, 0])
    for order in (1, 0):
        def run_split():
            cw = G.Context(rt, rt.ggml_tensor_overhead() * 4, no_alloc=True)
            cx = G.Context(rt, rt.ggml_tensor_overhead() * 8 + rt.ggml_graph_overhead(), no_alloc=True)
            try:
                w = rt.ggml_new_tensor_2d(cw.ctx, T, K, N)
                wbuf = rt.ggml_backend_alloc_ctx_tensors_from_buft(cw.ctx, buft)
                assert wbuf and rt.ggml_backend_buffer_name(wbuf) == b"MI355X_Split"
                xt = rt.ggml_new_tensor_2d(cx.ctx, G.GGML_TYPE_F32, K, B)
                y = rt.ggml_mul_mat(cx.ctx, w, xt)
                g = rt.ggml_new_graph(cx.ctx)
                rt.ggml_build_forward_expand(g, y)
                xbuf = rt.ggml_backend_alloc_ctx_tensors(cx.ctx, backend)
                try:
                    G.tensor_set(rt, w, wq)
                    back = np.empty_like(wq)
                    rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
                    assert np.array_equal(back, wq), "split set/get round trip"
                    G.tensor_set(rt, xt, x)
                    assert rt.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                    return G.tensor_get(rt, y)
                finally:
                    rt.ggml_backend_buffer_free(xbuf)
                    rt.ggml_backend_buffer_free(wbuf)
            finally:
                cx.free()
                cw.free()

        ys = in_order(rt, order, run_split)
        yu = in_order(rt, order, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        if order:
            assert same_bits(ys, yu), rel_err(ys, yu)
        else:
            assert rel_err(ys, yu) <= TREE_TOL, rel_err(ys, yu)


def test_gguf_iq4_weights_on_mi355x(rt, backend, tmp_path):
    """A GGUF file with a tensor of each type -> MI355X buffer (gguf.Model): the bytes arrive and
    MUL_MAT returns the golden outputs."""
    c = MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wqs = {T: golden_blob(f"{TAG[T]}_w.wq.bin") for T in (IQ4_NL, IQ4_XS)}
    path = str(tmp_path / "iq4.gguf")
    gguf.write(rt, path, [("general.architecture", "str", "test")],
               [("pad", G.GGML_TYPE_F32, [3], np.zeros(3, np.float32)), ("wnl", IQ4_NL, [K, N], wqs[IQ4_NL]),
                ("wxs", IQ4_XS, [K, N], wqs[IQ4_XS])])
    m = gguf.Model(rt, path, backend)
    try:
        x = synth.uniform(c["xseed"], K * B)
        for T, name in ((IQ4_NL, "wnl"), (IQ4_XS, "wxs")):
            w = m.tensors[name]
            assert w.contents.type == T
            back = np.empty(rt.ggml_nbytes(w), np.uint8)
            rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
            assert np.array_equal(back, wqs[T])

            def build(ctx):
                xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
                return [(xt, x)], rt.ggml_mul_mat(ctx, w, xt)

            y = in_order(rt, 1, lambda: G.graph_once(rt, backend, build))
            assert same_bits(y, golden_blob(f"{TAG[T]}_w.y.f32", np.float32)), name
    finally:
        m.free()
