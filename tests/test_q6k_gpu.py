"""GPU tests of Q6_K weights on the MI355X backend: GET_ROWS, MUL_MAT in the reference CPU's
summation order (mmv_order=1: identical bits) and in tree order (mmv_order=0: within 1e-5), the
default order of a quantized graph, a tiny Q6_K GPT-2 end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/q6k_* where those
suffice. All the assertions are path-agnostic: they hold whichever kernel serves a shape.
"""
import ctypes
import functools
import json
import os
import subprocess

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
REF_QUANTIZE = os.path.join(REF, "gpt-2-quantize")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference lib not built (make -C oracle ref)")
Q6_K, Q8_K = 14, 15
TREE_TOL = 1e-5  # integer block sums are exact: only the f32 combination order differs

with open(os.path.join(GOLDEN, "q6k.json")) as _f:
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
def weights(K, N, seed):
    """Seeded Q6_K rows from the runtime's quantizer (tests/test_q6k.py pins it to the reference's bytes)."""
    rt = G.runtime()
    w = np.random.default_rng(seed).standard_normal(K * N).astype(np.float32)
    out = np.empty(G.row_size(Q6_K, K) * N, np.uint8)
    assert rt.ggml_quantize_chunk(Q6_K, w.ctypes.data, out.ctypes.data, 0, N, K, None) == out.nbytes
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ GET_ROWS

@pytest.mark.parametrize("which", ["w", "edge"])
def test_get_rows_matches_golden_dequantization(rt, backend, which):
    """Row indices out of order and repeated, f32 dst: dequantize_row_q6_K's bits."""
    K, N = MANIFEST[which]["K"], MANIFEST[which]["N"]
    wq = golden_blob(f"q6k_{which}.wq.bin")
    want = golden_blob(f"q6k_{which}.wdq.f32", np.float32).reshape(N, K)
    idx = np.array([N - 1, 0, 2, 2, 1, N - 1, 3, 0, N - 2], np.int32)

    def build(c):
        w = rt.ggml_new_tensor_2d(c, Q6_K, K, N)
        i = rt.ggml_new_tensor_1d(c, G.GGML_TYPE_I32, len(idx))
        return [(w, wq), (i, idx)], rt.ggml_get_rows(c, w, i)

    y = G.graph_once(rt, backend, build).reshape(len(idx), K)
    assert same_bits(y, want[idx]), float(np.abs(y - want[idx]).max())


# ------------------------------------------------------------------ MUL_MAT

def test_mul_mat_matches_golden_output(rt, backend):
    """The committed reference-CPU output (B = 3): identical bits in order 1, 1e-5 in tree order."""
    c = MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wq = golden_blob("q6k_w.wq.bin")
    x = synth.uniform(c["xseed"], K * B)
    want = golden_blob("q6k_w.y.f32", np.float32)
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
    print(f"golden B={B}: order 1 rel err {rel_err(y1, want):.2e}, tree order {rel_err(y0, want):.2e}")
    assert same_bits(y1, want), rel_err(y1, want)
    assert rel_err(y0, want) <= TREE_TOL


# rows of 2 mod 4 alignment (odd superblock counts 1, 3, 11), under one / exactly one / one and a
# half items per lane of a wave (K 2048 / 4096 / 6144), N not a multiple of 4 or of the rows per
# workgroup, 1..8 columns in one launch, the 4-column split, 8-column chunks with a ragged tail
SHAPES = [(256, 5), (768, 67), (2048, 67), (2816, 33), (4096, 67), (6144, 9)]
COLS = [1, 2, 3, 5, 8, 9, 17]


@functools.lru_cache(maxsize=None)
def _ref_mul_mat(K, N, B):
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    try:
        y = G.mul_mat_once(lib, cpu, Q6_K, weights(K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)
    finally:
        lib.ggml_backend_free(cpu)
    y.setflags(write=False)
    return y


@needs_ref
@pytest.mark.parametrize("K,N", SHAPES)
def test_mul_mat_reference_order_bit_identical(rt, backend, K, N):
    wq = weights(K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        yr = _ref_mul_mat(K, N, B)
        assert same_bits(y, yr), (B, float(np.mean(y.view(np.uint32) == yr.view(np.uint32))), rel_err(y, yr))


@needs_ref
@pytest.mark.parametrize("K,N", SHAPES)
def test_mul_mat_tree_order(rt, backend, K, N):
    wq = weights(K, N, 100 + K + N)
    for B in COLS:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        err = rel_err(y, _ref_mul_mat(K, N, B))
        print(f"tree order K={K} N={N} B={B}: rel err {err:.2e}")
        assert err <= TREE_TOL, (B, err)


@needs_ref
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref):
    """K = 11008 (LLaMA-7B's ffn_down): 43 superblocks, 9030-byte rows -- every other row starts
    2 mod 4 -- and 172 items per row, more than two per lane. Decode and prompt column counts."""
    lib, cpu = ref
    K, N = 11008, 10
    wq = weights(K, N, 801)
    for B in (1, 3, 8, 9):
        x = synth.uniform(802 + B, K * B)
        yr = G.mul_mat_once(lib, cpu, Q6_K, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        assert same_bits(y1, yr), (B, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (B, rel_err(y0, yr))


def _mul_mat_general(lib, backend, wq, w_ne, x, x_ne, permute_x):
    """W [K, N, ne02, 1] x X [K, ne11, ne12, 1] with broadcasting; permute_x: X stored as
    [K, ne12, ne11] and permuted, so that src1's columns are strided."""
    ovh = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, ovh, no_alloc=True) as c:
        w = lib.ggml_new_tensor_4d(c.ctx, Q6_K, *w_ne)
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
def test_weight_batch_and_strided_src1(rt, backend, ref, ne11):
    """A 3-D weight batch (ne02 = 2) broadcast over ne12 = 4, contiguous and strided src1."""
    lib, cpu = ref
    K, N, ne02, ne12 = 512, 40, 2, 4
    w_ne, x_ne = (K, N, ne02, 1), (K, ne11, ne12, 1)
    wq = weights(K, N * ne02, 301)
    x = synth.uniform(302 + ne11, K * ne11 * ne12)
    for permute in (False, True):
        yr = _mul_mat_general(lib, cpu, wq, w_ne, x, x_ne, permute)
        y1 = in_order(rt, 1, lambda: _mul_mat_general(rt, backend, wq, w_ne, x, x_ne, permute))
        y0 = in_order(rt, 0, lambda: _mul_mat_general(rt, backend, wq, w_ne, x, x_ne, permute))
        assert same_bits(y1, yr), (permute, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (permute, rel_err(y0, yr))


def _cpy_q8k_then_mul_mat(lib, backend, wq, K, N, x, B):
    """X (f32) -> CPY to Q8_K rows -> MUL_MAT(W, Xq) as one graph: src1 already of the vec_dot type."""
    overhead = lib.ggml_tensor_overhead() * 8 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        w = lib.ggml_new_tensor_2d(c.ctx, Q6_K, K, N)
        xt = lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, B)
        xq = lib.ggml_cpy(c.ctx, xt, lib.ggml_new_tensor_2d(c.ctx, Q8_K, K, B))
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
def test_prequantized_q8k_src1(rt, backend, ref, B):
    lib, cpu = ref
    K, N = 1024, 48
    wq = weights(K, N, 401)
    x = synth.uniform(402 + B, K * B)
    yr = _cpy_q8k_then_mul_mat(lib, cpu, wq, K, N, x, B)
    y1 = in_order(rt, 1, lambda: _cpy_q8k_then_mul_mat(rt, backend, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: _cpy_q8k_then_mul_mat(rt, backend, wq, K, N, x, B))
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


def _three_mul_mats(lib, backend, wqs, K, N, xs):
    """Three independent same-shape mul_mats (B = 1) in one graph."""
    overhead = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        ws = [lib.ggml_new_tensor_2d(c.ctx, Q6_K, K, N) for _ in wqs]
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
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref):
    lib, cpu = ref
    K, N = 4096, 64
    wqs = [weights(K, N, 500 + i) for i in range(3)]
    xs = [synth.uniform(510 + i, K) for i in range(3)]
    yr = _three_mul_mats(lib, cpu, wqs, K, N, xs)
    y1 = in_order(rt, 1, lambda: _three_mul_mats(rt, backend, wqs, K, N, xs))
    y0 = in_order(rt, 0, lambda: _three_mul_mats(rt, backend, wqs, K, N, xs))
    for i in range(3):
        assert same_bits(y1[i], yr[i]), (i, rel_err(y1[i], yr[i]))
        assert rel_err(y0[i], yr[i]) <= TREE_TOL, (i, rel_err(y0[i], yr[i]))


def _block(ql, qh, scale, d=1.0):
    b = np.empty(210, np.uint8)
    b[:128] = ql
    b[128:192] = qh
    b[192:208] = np.array([scale], np.int8).view(np.uint8)[0]
    b[208:210] = np.array([d], np.float16).view(np.uint8)
    return b


@needs_ref
def test_extreme_integers(rt, backend, ref):
    """Hand-made blocks at the ends of the integer range -- every q - 32 = -32 under scales of -128
    (0x80), every q - 32 = 31 under scales of 127 -- against constant-valued columns, whose Q8_K
    quants are all of the largest magnitude (quantize_row_q8_K turns a constant column into -128
    throughout, one more than the +-127 of a mixed-sign one; the third superblock pairing below has
    alternating signs, so 127 occurs too). A reference lane sum then reaches 8 * 128 * 4 * 32 * 128 =
    2^24 exactly and a 64-element item sum twice that, beyond what f32 holds exactly: this pins the
    int32 accumulation. K = 512, N = 8, B = 2."""
    lib, cpu = ref
    lo, hi = _block(0x00, 0x00, -128), _block(0xFF, 0xFF, 127)
    pairs = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    wq = np.concatenate([np.concatenate(p) for p in pairs + pairs[::-1]])
    K, N, B = 512, 8, 2
    assert wq.size == N * G.row_size(Q6_K, K)
    for x in (np.concatenate([np.full(K, 0.5, np.float32), np.full(K, -2.0, np.float32)]),
              np.concatenate([np.tile(np.array([3.0, -3.0], np.float32), K // 2), np.full(K, 1e-3, np.float32)])):
        yr = G.mul_mat_once(lib, cpu, Q6_K, wq, K, N, x, B)
        assert np.abs(yr).max() > 1.0  # the sums did not cancel
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        assert same_bits(y1, yr), (y1, yr)
        assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


@needs_ref
@pytest.mark.parametrize("B", [1, 3])
def test_default_order_of_a_quantized_chain(rt, backend, ref, B):
    """Q6_K . x -> RMSNorm -> Q6_K with the default settings (mmv_order -1): the second mul_mat
    consumes computed activations, so the graph runs in the reference order -- the reference CPU's bits."""
    lib, cpu = ref
    K, N1, N2 = 1024, 768, 37
    w1, w2 = weights(K, N1, 601), weights(N1, N2, 602)
    x = synth.uniform(603 + B, K * B)

    def build(L, c):
        a = L.ggml_new_tensor_2d(c, Q6_K, K, N1)
        b = L.ggml_new_tensor_2d(c, Q6_K, N1, N2)
        xt = L.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, B)
        h = L.ggml_rms_norm(c, L.ggml_mul_mat(c, a, xt), 1e-5)
        return [(a, w1), (b, w2), (xt, x)], L.ggml_mul_mat(c, b, h)

    y = G.graph_once(rt, backend, lambda c: build(rt, c))
    yr = G.graph_once(lib, cpu, lambda c: build(lib, c))
    assert same_bits(y, yr), rel_err(y, yr)


# ------------------------------------------------------------------ GPT-2 end to end

TINY = dict(n_embd=256, n_head=4, n_layer=2, n_vocab=512, n_ctx=64)


@pytest.fixture(scope="module")
def tiny_q6k(tmp_path_factory):
    d = tmp_path_factory.mktemp("q6k_gpt2")
    f16 = gpt2.write_synthetic_model(str(d / "tiny-f16.bin"), **TINY)
    return f16, gpt2.quantize_model(G.runtime(), f16, str(d / "tiny-q6_k.bin"), "q6_k")


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
def test_quantized_model_file_matches_reference_program(tiny_q6k, tmp_path):
    import filecmp
    f16, ours = tiny_q6k
    out = str(tmp_path / "ref-q6_k.bin")
    p = subprocess.run([REF_QUANTIZE, f16, out, "q6_k"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(ours) == os.path.getsize(out)
    assert filecmp.cmp(ours, out, shallow=False)


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
def test_gpt2_q6k_logits_bit_identical_to_reference_cpu(tiny_q6k, mode):
    """A tiny Q6_K GPT-2 (Q6_K get_rows embedding, Q6_K MUL_MAT for every projection and the lm_head),
    default settings: teacher-forced decode over 12 tokens, a 20-token prompt in one batch (the
    chunked > 8 column path) and a prompt in batches of 8 -- the reference CPU's logits, bit for bit."""
    n_batch = 20 if mode == "prompt20" else 8
    ours, rm, free = _both_models(tiny_q6k[1], n_batch)
    try:
        assert ours.hp.ftype % 1000 == 14
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
def test_split_buffer_weights(rt, backend, B):
    """Q6_K rows divided over the slots of a split buffer (slots beyond the device count are virtual
    slots on device 0, each with its own allocation, stream and copies): each slice runs through the
    same mul_mat as the unsplit weight: the unsplit result's bits in the reference order, within
    1e-5 of it in tree order."""
    K, N = 768, 333  # 630-byte rows: slices start 2 mod 4
    wq = weights(K, N, 701)
    x = synth.uniform(702 + B, K * B)
    buft = _split_buft(rt, [1, 1, 0])
    for order in (1, 0):
        def run_split():
            cw = G.Context(rt, rt.ggml_tensor_overhead() * 4, no_alloc=True)
            cx = G.Context(rt, rt.ggml_tensor_overhead() * 8 + rt.ggml_graph_overhead(), no_alloc=True)
            try:
                w = rt.ggml_new_tensor_2d(cw.ctx, Q6_K, K, N)
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
        yu = in_order(rt, order, lambda: G.mul_mat_once(rt, backend, Q6_K, wq, K, N, x, B))
        if order:
            assert same_bits(ys, yu), rel_err(ys, yu)
        else:
            assert rel_err(ys, yu) <= TREE_TOL, rel_err(ys, yu)


def test_gguf_q6k_weights_on_mi355x(rt, backend, tmp_path):
    """A GGUF file with a Q6_K tensor -> MI355X buffer (gguf.Model): the bytes arrive, GET_ROWS
    returns the golden dequantization and MUL_MAT the golden output."""
    c = MANIFEST["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wq = golden_blob("q6k_w.wq.bin")
    path = str(tmp_path / "q6k.gguf")
    gguf.write(rt, path, [("general.architecture", "str", "test")],
               [("pad", G.GGML_TYPE_F32, [3], np.zeros(3, np.float32)), ("w", Q6_K, [K, N], wq)])
    m = gguf.Model(rt, path, backend)
    try:
        w = m.tensors["w"]
        assert w.contents.type == Q6_K
        back = np.empty(rt.ggml_nbytes(w), np.uint8)
        rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
        assert np.array_equal(back, wq)
        x = synth.uniform(c["xseed"], K * B)

        def build(ctx):
            xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
            return [(xt, x)], rt.ggml_mul_mat(ctx, w, xt)

        y = in_order(rt, 1, lambda: G.graph_once(rt, backend, build))
        assert same_bits(y, golden_blob("q6k_w.y.f32", np.float32))
    finally:
        m.free()
