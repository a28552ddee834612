"""GPU tests of Q4_1 / Q5_0 / Q5_1 weights (and Q8_1 activations) on the MI355X backend: GET_ROWS,
the activation quantizer, MUL_MAT in the reference CPU's summation order (mmv_order=1: identical
bits) and in tree order (mmv_order=0: within 1e-5), the default order of a quantized graph, a tiny
GPT-2 of each type end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/legacy_* where those
suffice. The bodies that other types share are the check_* functions of tests/weight_types.py, run
on the table's Q4_1, Q5_0 and Q5_1 rows.
"""
import os

import numpy as np
import pytest

import weight_types as W
from conftest import golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import synth
from weight_types import Q8_1, REF_GPT2, TREE_TOL, in_order, needs_ref, rel_err, same_bits
from weight_types import backend, ref, rt, tiny_models  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROWS = W.rows("legacy")
by_type = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)


@pytest.mark.parametrize("which", ["w", "edge"])
@by_type
def test_get_rows_matches_golden_dequantization(rt, backend, wt, which):
    W.check_get_rows_matches_golden_dequantization(rt, backend, wt, which)


def test_q8_1_activation_quantizer_matches_golden_rows(rt, backend):
    """The device quantizer MUL_MAT uses for Q4_1 / Q5_1 weights: quantize_row_q8_1's quants, d and s."""
    c = ROWS[0].manifest["w"]
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
    c = ROWS[0].manifest["w"]
    K, B = c["K"], c["B"]
    x = synth.uniform(c["xseed"], K * B)

    def build(ctx):
        xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
        return [(xt, x)], rt.ggml_cpy(ctx, xt, rt.ggml_new_tensor_2d(ctx, Q8_1, K, B))

    out = G.graph_once(rt, backend, build).view(np.uint8)
    assert np.array_equal(out, golden_blob("legacy_x.xq.bin"))


@by_type
def test_mul_mat_matches_golden_output(rt, backend, wt):
    W.check_mul_mat_matches_golden_output(rt, backend, wt)


@needs_ref
@pytest.mark.parametrize("K,N", ROWS[0].shapes)
@by_type
def test_mul_mat_reference_order_bit_identical(rt, backend, wt, K, N):
    W.check_mul_mat_reference_order_bit_identical(rt, backend, wt, (K, N))


@needs_ref
@pytest.mark.parametrize("K,N", ROWS[0].shapes)
@by_type
def test_mul_mat_tree_order(rt, backend, wt, K, N):
    W.check_mul_mat_tree_order(rt, backend, wt, (K, N))


@needs_ref
@by_type
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref, wt):
    W.check_mul_mat_llama_ffn_down_rows(rt, backend, ref, wt)


@needs_ref
@pytest.mark.parametrize("ne11", [1, 3, 9])
@by_type
def test_weight_batch_and_strided_src1(rt, backend, ref, wt, ne11):
    W.check_weight_batch_and_strided_src1(rt, backend, ref, wt, ne11)


@needs_ref
@pytest.mark.parametrize("B", ROWS[0].prequant_B)
@by_type
def test_prequantized_src1(rt, backend, ref, wt, B):
    W.check_prequantized_src1(rt, backend, ref, wt, B)


@needs_ref
@by_type
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref, wt):
    W.check_three_independent_mul_mats_in_one_graph(rt, backend, ref, wt)


def _one_hot_qs(byte, value):
    qs = np.zeros(16, np.uint8)
    qs[byte] = value
    return qs


def _hand_made_kinds(wt):
    """lo, hi: a single fifth bit over zero nibbles for a low-half (5) and a high-half (21) element
    (Q4_1, which has none: a single nibble); all nibbles and bits set; all zeros (Q5_0: every q - 16 = -16)."""
    if wt.tag == "q4_1":
        lo, hi = wt.block(_one_hot_qs(5, 0x0F)), wt.block(_one_hot_qs(5, 0xF0))
    else:
        lo, hi = wt.block(0x00, 1 << 5), wt.block(0x00, 1 << 21)
    return lo, hi, wt.block(0xFF, 0xFFFFFFFF, d=0.75, m=-1.5), wt.block(0x00, 0, d=2.0, m=0.25)


@needs_ref
@by_type
def test_hand_made_blocks(rt, backend, ref, wt):
    """Blocks that pin the bit -> element mapping and the ends of the integer range (_hand_made_kinds)
    against a seeded column, a constant column (whose quants are all 127) and one of alternating
    signs. K = 64, N = 6, B = 3."""
    lib, cpu = ref
    t = wt.type
    lo, hi, full, zero = _hand_made_kinds(wt)
    pairs = [(lo, hi), (hi, lo), (full, full), (zero, zero), (full, zero), (lo, full)]
    wq = np.concatenate([np.concatenate(p) for p in pairs])
    K, N, B = 64, len(pairs), 3
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
def test_hand_made_blocks_streaming_shape(rt, backend, ref, wt):
    """The same hand-made blocks tiled to K = 512 (16-byte aligned rows: the streaming kernel's shapes), B = 1 and 3."""
    lib, cpu = ref
    t = wt.type
    kinds = _hand_made_kinds(wt)
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
@pytest.mark.parametrize("B", ROWS[0].chain_B)
@by_type
def test_default_order_of_a_quantized_chain(rt, backend, ref, wt, B):
    W.check_default_order_of_a_quantized_chain(rt, backend, ref, wt, B)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("mode", ROWS[0].gpt2_modes)
@by_type
def test_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode):
    W.check_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode)


@pytest.mark.parametrize("B", ROWS[0].split_B)
@by_type
def test_split_buffer_weights(rt, backend, wt, B):
    W.check_split_buffer_weights(rt, backend, wt, B)


def test_gguf_weights_on_mi355x(rt, backend, tmp_path):
    W.check_gguf_weights_on_mi355x(rt, backend, tmp_path, "legacy")
