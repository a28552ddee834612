"""GPU tests of Q4_1 / Q5_0 / Q5_1 weights (and Q8_1 activations) on the MI355X backend: GET_ROWS,
the activation quantizer, MUL_MAT in the reference CPU's summation order (mmv_order=1: identical
bits) and in tree order (mmv_order=0: within 1e-5), the default order of a quantized graph, a tiny
GPT-2 of each type end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/legacy_* where those
suffice. All the assertions are path-agnostic: they hold whichever kernel serves a shape.
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
TYPES = {"q4_1": 3, "q5_0": 6, "q5_1": 7}
BLOCK_BYTES = {3: 20, 6: 22, 7: 24}
FTYPE = {"q4_1": 3, "q5_0": 8, "q5_1": 9}
NAMES = sorted(TYPES)
Q8_0, Q8_1 = 8, 9
TREE_TOL = 1e-5  # integer block sums are exact: only the f32 combination order differs

with open(os.path.join(GOLDEN, "legacy.json")) as _f:
    MANIFEST = json.load(_f)

by_type = pytest.mark.parametrize("name", NAMES)


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
def weights(t, K, N, seed):
    """Seeded rows from the runtime's quantizer (tests/test_legacy_quants.py pins it to the reference's bytes)."""
    rt = G.runtime()
    w = np.random.default_rng(seed).standard_normal(K * N).astype(np.float32)
    out = np.empty(G.row_size(t, K) * N, np.uint8)
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, N, K, None) == out.nbytes
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ GET_ROWS

@pytest.mark.parametrize("which", ["w", "edge"])
@by_type
def test_get_rows_matches_golden_dequantization(rt, backend, name, which):
    """Row indices out of order and repeated, f32 dst: dequantize_row_*'s bits."""
    t, K, N = TYPES[name], MANIFEST[which]["K"], MANIFEST[which]["N"]
    wq = golden_blob(f"legacy_{name}_{which}.wq.bin")
    want = golden_blob(f"legacy_{name}_{which}.wdq.f32", np.float32).reshape(N, K)
    idx = np.array([N - 1, 0, 2, 2, 1, N - 1, 3, 0, N - 2], np.int32)

    def build(c):
        w = rt.ggml_new_tensor_2d(c, t, K, N)
        i = rt.ggml_new_tensor_1d(c, G.GGML_TYPE_I32, len(idx))
        return [(w, wq), (i, idx)], rt.ggml_get_rows(c, w, i)

    y = G.graph_once(rt, backend, build).reshape(len(idx), K)
    assert same_bits(y, want[idx]), float(np.abs(y - want[idx]).max())


# ------------------------------------------------------------------ Q8_1 activations

def test_q8_1_activation_quantizer_matches_golden_rows(rt, backend):
    """The device quantizer MUL_MAT uses for Q4_1 / Q5_1 weights: quantize_row_q8_1's quants, d and s."""
    c = MANIFEST["w"]
    K, B = c["K"], c["B"]
    x = synth.uniform(c["xseed"], K * B)
    want = golden_blob("legacy_x.xq.bin").reshape(B * K // 32, 36)
    qs = np.empty(K * B, np.int8)
    d = np.empty(K // 32 * B, np.float32)
    s = np.empty(K // 32 * B, np.int16)
    assert rt.ggml_backend_mi355x_quantize_activations(backend, Q8_1, x.ctypes.data, K, B, qs.ctypes.data, d.ctypes.data, s.ctypes.data)
    assert np.array_equal(qs.reshape(-1, 32).view(np.uint8), want[:, 4:])
    assert np.array_equal(d.astype(np.float16).view(np.uint16), want[:, 0:2].copy().view(np.uint16).ravel())
    assert np.array_equal(d.astype(np.float16).astype(np.float32), d)  # the fp16-rounded d
    assert np.array_equal(s.view(np.uint16), want[:, 2:4].copy().view(np.uint16).ravel())


def test_cpy_f32_to_q8_1_matches_golden_rows(rt, backend):
    """GGML_OP_CPY F32 -> Q8_1 writes block_q8_1 rows: the reference's bytes."""
    c = MANIFEST["w"]
    K, B = c["K"], c["B"]
    x = synth.uniform(c["xseed"], K * B)

    def build(ctx):
        xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
        return [(xt, x)], rt.ggml_cpy(ctx, xt, rt.ggml_new_tensor_2d(ctx, Q8_1, K, B))

    out = G.graph_once(rt, backend, build).view(np.uint8)
    assert np.array_equal(out, golden_blob("legacy_x.xq.bin"))


# ------------------------------------------------------------------ MUL_MAT

@by_type
def test_mul_mat_matches_golden_output(rt, backend, name):
    """The committed reference-CPU output (B = 3): identical bits in order 1, 1e-5 in tree order."""
    t, c = TYPES[name], MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wq = golden_blob(f"legacy_{name}_w.wq.bin")
    x = synth.uniform(c["xseed"], K * B)
    want = golden_blob(f"legacy_{name}_w.y.f32", np.float32)
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
    print(f"{name} golden B={B}: order 1 rel err {rel_err(y1, want):.2e}, tree order {rel_err(y0, want):.2e}")
    assert same_bits(y1, want), rel_err(y1, want)
    assert rel_err(y0, want) <= TREE_TOL


# one block; ragged K (3 blocks); an odd block count whose Q5_0 rows are 2 mod 4 (25 blocks = 550 B);
# under one, exactly one and one and a half blocks per lane pair of a wave (K 2048 / 4096 / 6144); N
# not a multiple of the rows per workgroup; 1..8 columns in one launch, the 4-column split, 8-column
# chunks with a ragged tail
SHAPES = [(32, 5), (96, 67), (800, 33), (2048, 67), (4096, 67), (6144, 9)]
COLS = [1, 2, 3, 5, 8, 9, 17]


@functools.lru_cache(maxsize=None)
def _ref_mul_mat(t, K, N, B):
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    try:
        y = G.mul_mat_once(lib, cpu, t, weights(t, K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)
    finally:
        lib.ggml_backend_free(cpu)
    y.setflags(write=False)
    return y


@needs_ref
@pytest.mark.parametrize("K,N", SHAPES)
@by_type
def test_mul_mat_reference_order_bit_identical(rt, backend, name, K, N):
    t = TYPES[name]
    wq = weights(t, K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        yr = _ref_mul_mat(t, K, N, B)
        assert same_bits(y, yr), (B, float(np.mean(y.view(np.uint32) == yr.view(np.uint32))), rel_err(y, yr))


@needs_ref
@pytest.mark.parametrize("K,N", SHAPES)
@by_type
def test_mul_mat_tree_order(rt, backend, name, K, N):
    t = TYPES[name]
    wq = weights(t, K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        err = rel_err(y, _ref_mul_mat(t, K, N, B))
        print(f"{name} tree order K={K} N={N} B={B}: rel err {err:.2e}")
        assert err <= TREE_TOL, (B, err)


@needs_ref
@by_type
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref, name):
    """K = 11008 (LLaMA-7B's ffn_down): 344 blocks a row, more than five per lane; not a multiple of
    256, so the generic kernels serve it. Decode and prompt column counts."""
    lib, cpu = ref
    t, K, N = TYPES[name], 11008, 10
    wq = weights(t, K, N, 801)
    for B in (1, 3, 8, 9):
        x = synth.uniform(802 + B, K * B)
        yr = G.mul_mat_once(lib, cpu, t, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        assert same_bits(y1, yr), (B, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (B, rel_err(y0, yr))


def _mul_mat_general(lib, backend, t, wq, w_ne, x, x_ne, permute_x):
    """W [K, N, ne02, 1] x X [K, ne11, ne12, 1] with broadcasting; permute_x: X stored as
    [K, ne12, ne11] and permuted, so that src1's columns are strided."""
    ovh = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, ovh, no_alloc=True) as c:
        w = lib.ggml_new_tensor_4d(c.ctx, t, *w_ne)
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
@pytest.mark.parametrize("ne11", [1, 3, 9])
@by_type
def test_weight_batch_and_strided_src1(rt, backend, ref, name, ne11):
    """A 3-D weight batch (ne02 = 2) broadcast over ne12 = 4, contiguous and strided src1."""
    lib, cpu = ref
    t, K, N, ne02, ne12 = TYPES[name], 512, 40, 2, 4
    w_ne, x_ne = (K, N, ne02, 1), (K, ne11, ne12, 1)
    wq = weights(t, K, N * ne02, 301)
    x = synth.uniform(302 + ne11, K * ne11 * ne12)
    for permute in (False, True):
        yr = _mul_mat_general(lib, cpu, t, wq, w_ne, x, x_ne, permute)
        y1 = in_order(rt, 1, lambda: _mul_mat_general(rt, backend, t, wq, w_ne, x, x_ne, permute))
        y0 = in_order(rt, 0, lambda: _mul_mat_general(rt, backend, t, wq, w_ne, x, x_ne, permute))
        assert same_bits(y1, yr), (permute, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (permute, rel_err(y0, yr))


def _cpy_then_mul_mat(lib, backend, t, wq, K, N, x, B):
    """X (f32) -> CPY to rows of the weight's vec_dot type -> MUL_MAT(W, Xq) as one graph."""
    overhead = lib.ggml_tensor_overhead() * 8 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        w = lib.ggml_new_tensor_2d(c.ctx, t, K, N)
        xt = lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, B)
        xq = lib.ggml_cpy(c.ctx, xt, lib.ggml_new_tensor_2d(c.ctx, Q8_0 if t == 6 else Q8_1, K, B))
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
@pytest.mark.parametrize("B", [4, 20])
@by_type
def test_prequantized_src1(rt, backend, ref, name, B):
    """src1 already of the vec_dot type (Q5_0: Q8_0 rows; Q4_1 / Q5_1: Q8_1 rows), read as it lies."""
    lib, cpu = ref
    t, K, N = TYPES[name], 1024, 48
    wq = weights(t, K, N, 401)
    x = synth.uniform(402 + B, K * B)
    yr = _cpy_then_mul_mat(lib, cpu, t, wq, K, N, x, B)
    y1 = in_order(rt, 1, lambda: _cpy_then_mul_mat(rt, backend, t, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: _cpy_then_mul_mat(rt, backend, t, wq, K, N, x, B))
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


def _three_mul_mats(lib, backend, t, wqs, K, N, xs):
    """Three independent same-shape mul_mats (B = 1) in one graph."""
    overhead = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        ws = [lib.ggml_new_tensor_2d(c.ctx, t, K, N) for _ in wqs]
        xts = [lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, 1) for _ in xs]
        ys = [lib.ggml_mul_mat(c.ctx, w, x) for w, x in zip(ws, xts)]
        g = lib.ggml_new_graph(c.ctx)
        for y in ys:
            lib.ggml_build_forward_expand(g, y)
        buf = lib.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf
        try:
            for tt, a in list(zip(ws, wqs)) + list(zip(xts, xs)):
                G.tensor_set(lib, tt, a)
            assert lib.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return [G.tensor_get(lib, y) for y in ys]
        finally:
            lib.ggml_backend_buffer_free(buf)


@needs_ref
@by_type
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref, name):
    lib, cpu = ref
    t, K, N = TYPES[name], 4096, 64
    wqs = [weights(t, K, N, 500 + i) for i in range(3)]
    xs = [synth.uniform(510 + i, K) for i in range(3)]
    yr = _three_mul_mats(lib, cpu, t, wqs, K, N, xs)
    y1 = in_order(rt, 1, lambda: _three_mul_mats(rt, backend, t, wqs, K, N, xs))
    y0 = in_order(rt, 0, lambda: _three_mul_mats(rt, backend, t, wqs, K, N, xs))
    for i in range(3):
        assert same_bits(y1[i], yr[i]), (i, rel_err(y1[i], yr[i]))
        assert rel_err(y0[i], yr[i]) <= TREE_TOL, (i, rel_err(y0[i], yr[i]))


def _block(t, qs, qh=0, d=1.0, m=0.5):
    """One hand-made block: qs 16 bytes (or one value for all), qh the 32 fifth bits."""
    parts = [np.array([d], np.float16).view(np.uint8)]
    if t != 6:
        parts.append(np.array([m], np.float16).view(np.uint8))
    if t != 3:
        parts.append(np.array([qh], "<u4").view(np.uint8))
    parts.append(np.broadcast_to(np.asarray(qs, np.uint8), (16,)))
    b = np.concatenate(parts)
    assert b.size == BLOCK_BYTES[t]
    return b


def _one_hot_qs(byte, value):
    qs = np.zeros(16, np.uint8)
    qs[byte] = value
    return qs


@needs_ref
@by_type
def test_hand_made_blocks(rt, backend, ref, name):
    """Blocks that pin the bit -> element mapping and the ends of the integer range: a single fifth
    bit over zero nibbles for a low-half (5) and a high-half (21) element (Q4_1, which has none: a
    single nibble), all nibbles and bits set, and all zeros (Q5_0: every q - 16 = -16) -- against a
    seeded column, a constant column (whose quants are all 127) and one of alternating signs.
    K = 64, N = 6, B = 3."""
    lib, cpu = ref
    t = TYPES[name]
    if t == 3:
        lo, hi = _block(t, _one_hot_qs(5, 0x0F)), _block(t, _one_hot_qs(5, 0xF0))
    else:
        lo, hi = _block(t, 0x00, 1 << 5), _block(t, 0x00, 1 << 21)
    full, zero = _block(t, 0xFF, 0xFFFFFFFF, d=0.75, m=-1.5), _block(t, 0x00, 0, d=2.0, m=0.25)
    rows = [(lo, hi), (hi, lo), (full, full), (zero, zero), (full, zero), (lo, full)]
    wq = np.concatenate([np.concatenate(p) for p in rows])
    K, N, B = 64, len(rows), 3
    assert wq.size == N * G.row_size(t, K)
    x = np.concatenate([synth.uniform(901, K), np.full(K, 0.5, np.float32), np.tile(np.array([3.0, -3.0], np.float32), K // 2)])
    yr = G.mul_mat_once(lib, cpu, t, wq, K, N, x, B)
    assert np.abs(yr).max() > 1.0  # the sums did not cancel
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
    assert same_bits(y1, yr), (y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
    # the same rows through GET_ROWS: the reference's dequantization, element for element
    idx = np.arange(N, dtype=np.int32)

    def build(L, c):
        w = L.ggml_new_tensor_2d(c, t, K, N)
        i = L.ggml_new_tensor_1d(c, G.GGML_TYPE_I32, N)
        return [(w, wq), (i, idx)], L.ggml_get_rows(c, w, i)

    assert same_bits(G.graph_once(rt, backend, lambda c: build(rt, c)), G.graph_once(lib, cpu, lambda c: build(lib, c)))


@needs_ref
@by_type
def test_hand_made_blocks_streaming_shape(rt, backend, ref, name):
    """The same hand-made blocks tiled to K = 512 (16-byte aligned rows: the streaming kernel's shapes), B = 1 and 3."""
    lib, cpu = ref
    t = TYPES[name]
    if t == 3:
        lo, hi = _block(t, _one_hot_qs(5, 0x0F)), _block(t, _one_hot_qs(5, 0xF0))
    else:
        lo, hi = _block(t, 0x00, 1 << 5), _block(t, 0x00, 1 << 21)
    full, zero = _block(t, 0xFF, 0xFFFFFFFF, d=0.75, m=-1.5), _block(t, 0x00, 0, d=2.0, m=0.25)
    kinds = [lo, hi, full, zero]
    K, N = 512, 8
    wq = np.concatenate([kinds[(r + b) % 4] if r < 4 else kinds[r - 4] for r in range(N) for b in range(K // 32)])
    assert wq.size == N * G.row_size(t, K)
    for B in (1, 3):
        x = np.concatenate([synth.uniform(911, K), np.full(K, 0.5, np.float32), np.tile(np.array([3.0, -3.0], np.float32), K // 2)])[:K * B]
        yr = G.mul_mat_once(lib, cpu, t, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        assert same_bits(y1, yr), (B, y1, yr)
        assert rel_err(y0, yr) <= TREE_TOL, (B, rel_err(y0, yr))


@needs_ref
@pytest.mark.parametrize("B", [1, 3])
@by_type
def test_default_order_of_a_quantized_chain(rt, backend, ref, name, B):
    """W . x -> RMSNorm -> W with the default settings (mmv_order -1): the second mul_mat consumes
    computed activations, so the graph runs in the reference order -- the reference CPU's bits."""
    lib, cpu = ref
    t, K, N1, N2 = TYPES[name], 1024, 768, 37
    w1, w2 = weights(t, K, N1, 601), weights(t, N1, N2, 602)
    x = synth.uniform(603 + B, K * B)

    def build(L, c):
        a = L.ggml_new_tensor_2d(c, t, K, N1)
        b = L.ggml_new_tensor_2d(c, t, N1, N2)
        xt = L.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, B)
        h = L.ggml_rms_norm(c, L.ggml_mul_mat(c, a, xt), 1e-5)
        return [(a, w1), (b, w2), (xt, x)], L.ggml_mul_mat(c, b, h)

    y = G.graph_once(rt, backend, lambda c: build(rt, c))
    yr = G.graph_once(lib, cpu, lambda c: build(lib, c))
    assert same_bits(y, yr), rel_err(y, yr)


# ------------------------------------------------------------------ GPT-2 end to end

TINY = dict(n_embd=256, n_head=4, n_layer=2, n_vocab=512, n_ctx=64)


@pytest.fixture(scope="module")
def tiny_models(tmp_path_factory):
    d = tmp_path_factory.mktemp("legacy_gpt2")
    f16 = gpt2.write_synthetic_model(str(d / "tiny-f16.bin"), **TINY)
    return {name: gpt2.quantize_model(G.runtime(), f16, str(d / f"tiny-{name}.bin"), name) for name in NAMES}


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
@pytest.mark.parametrize("mode", ["decode", "prompt20", "batches_of_8"])
@by_type
def test_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, name, mode):
    """A tiny GPT-2 of the type (get_rows embedding, MUL_MAT for every projection and the lm_head),
    default settings: teacher-forced decode over 12 tokens, a 20-token prompt in one batch (the
    chunked > 8 column path) and a prompt in batches of 8 -- the reference CPU's logits, bit for bit."""
    n_batch = 20 if mode == "prompt20" else 8
    ours, rm, free = _both_models(tiny_models[name], n_batch)
    try:
        assert ours.hp.ftype % 1000 == FTYPE[name]
        if mode == "decode":
            steps = [[t] for t in TOKENS[:12]]
        elif mode == "prompt20":
            steps = [TOKENS]
        else:
            steps = [TOKENS[0:8], TOKENS[8:16], TOKENS[16:20]]
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


@pytest.mark.parametrize("B", [1, 12])
@by_type
def test_split_buffer_weights(rt, backend, name, B):
    """Rows divided over the slots of a split buffer (slots beyond the device count are virtual
    slots on device 0, each with its own allocation, stream and copies): each slice runs through the
    same mul_mat as the unsplit weight: the unsplit result's bits in the reference order, within
    1e-5 of it in tree order."""
    t, K, N = TYPES[name], 768, 333
    wq = weights(t, K, N, 701)
    x = synth.uniform(702 + B, K * B)
    buft = _split_buft(rt, [1, 1, 0])
    for order in (1, 0):
        def run_split():
            cw = G.Context(rt, rt.ggml_tensor_overhead() * 4, no_alloc=True)
            cx = G.Context(rt, rt.ggml_tensor_overhead() * 8 + rt.ggml_graph_overhead(), no_alloc=True)
            try:
                w = rt.ggml_new_tensor_2d(cw.ctx, t, K, N)
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
        yu = in_order(rt, order, lambda: G.mul_mat_once(rt, backend, t, wq, K, N, x, B))
        if order:
            assert same_bits(ys, yu), rel_err(ys, yu)
        else:
            assert rel_err(ys, yu) <= TREE_TOL, rel_err(ys, yu)


def test_gguf_weights_on_mi355x(rt, backend, tmp_path):
    """A GGUF file with a tensor of each type -> MI355X buffer (gguf.Model): the bytes arrive,
    GET_ROWS returns the golden dequantization and MUL_MAT the golden output."""
    c = MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wqs = {name: golden_blob(f"legacy_{name}_w.wq.bin") for name in NAMES}
    path = str(tmp_path / "legacy.gguf")
    gguf.write(rt, path, [("general.architecture", "str", "test")],
               [("pad", G.GGML_TYPE_F32, [3], np.zeros(3, np.float32))] + [(f"w_{name}", TYPES[name], [K, N], wqs[name]) for name in NAMES])
    m = gguf.Model(rt, path, backend)
    try:
        x = synth.uniform(c["xseed"], K * B)
        idx = np.array([N - 1, 0, 2, 2], np.int32)
        for name in NAMES:
            w = m.tensors[f"w_{name}"]
            assert w.contents.type == TYPES[name]
            back = np.empty(rt.ggml_nbytes(w), np.uint8)
            rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
            assert np.array_equal(back, wqs[name])

            def build_mm(ctx):
                xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
                return [(xt, x)], rt.ggml_mul_mat(ctx, w, xt)

            def build_gr(ctx):
                i = rt.ggml_new_tensor_1d(ctx, G.GGML_TYPE_I32, len(idx))
                return [(i, idx)], rt.ggml_get_rows(ctx, w, i)

            y = in_order(rt, 1, lambda: G.graph_once(rt, backend, build_mm))
            assert same_bits(y, golden_blob(f"legacy_{name}_w.y.f32", np.float32)), name
            rows = G.graph_once(rt, backend, build_gr).reshape(len(idx), K)
            want = golden_blob(f"legacy_{name}_w.wdq.f32", np.float32).reshape(N, K)
            assert same_bits(rows, want[idx]), name
    finally:
        m.free()
