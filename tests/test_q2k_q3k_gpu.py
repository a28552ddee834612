"""GPU tests of Q2_K and Q3_K weights on the MI355X backend: GET_ROWS, MUL_MAT and MUL_MAT_ID in the
reference CPU's summation order (mmv_order=1: identical bits) and in tree order (mmv_order=0: within
1e-5), the default order of a quantized graph, a tiny GPT-2 of each type end to end, split buffers
and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/q2k_*, q3k_* where
those suffice. The bodies are the check_* functions of tests/weight_types.py, run on the table's
Q2_K and Q3_K rows.
"""
import os

import pytest

import weight_types as W
from weight_types import REF_GPT2, REF_QUANTIZE, needs_ref
from weight_types import backend, ref, rt, tiny_models  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROWS = W.rows("q2k_q3k")
both_types = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)


@both_types
@pytest.mark.parametrize("which", ["w", "edge"])
def test_get_rows_matches_golden_dequantization(rt, backend, wt, which):
    W.check_get_rows_matches_golden_dequantization(rt, backend, wt, which)


@both_types
def test_mul_mat_matches_golden_output(rt, backend, wt):
    W.check_mul_mat_matches_golden_output(rt, backend, wt)


@needs_ref
@both_types
@pytest.mark.parametrize("K,N", ROWS[0].shapes)
def test_mul_mat_reference_order_bit_identical(rt, backend, wt, K, N):
    W.check_mul_mat_reference_order_bit_identical(rt, backend, wt, (K, N))


@needs_ref
@both_types
@pytest.mark.parametrize("K,N", ROWS[0].shapes)
def test_mul_mat_tree_order(rt, backend, wt, K, N):
    W.check_mul_mat_tree_order(rt, backend, wt, (K, N))


@needs_ref
@both_types
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref, wt):
    W.check_mul_mat_llama_ffn_down_rows(rt, backend, ref, wt)


@needs_ref
@both_types
@pytest.mark.parametrize("ne11", [1, 3, 9])
def test_weight_batch_and_strided_src1(rt, backend, ref, wt, ne11):
    W.check_weight_batch_and_strided_src1(rt, backend, ref, wt, ne11)


@needs_ref
@both_types
@pytest.mark.parametrize("B", ROWS[0].prequant_B)
def test_prequantized_q8k_src1(rt, backend, ref, wt, B):
    W.check_prequantized_src1(rt, backend, ref, wt, B)


@needs_ref
@both_types
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref, wt):
    W.check_three_independent_mul_mats_in_one_graph(rt, backend, ref, wt)


@needs_ref
@both_types
def test_extreme_integers(rt, backend, ref, wt):
    W.check_extreme_integers(rt, backend, ref, wt)


@needs_ref
@both_types
@pytest.mark.parametrize("B", ROWS[0].chain_B)
def test_default_order_of_a_quantized_chain(rt, backend, ref, wt, B):
    W.check_default_order_of_a_quantized_chain(rt, backend, ref, wt, B)


@needs_ref
@both_types
@pytest.mark.parametrize("n_tokens", ROWS[0].id_tokens)
def test_mul_mat_id_top2_of_4_experts(rt, backend, ref, wt, n_tokens):
    W.check_mul_mat_id_top2_of_4_experts(rt, backend, ref, wt, n_tokens)


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
@both_types
def test_quantized_model_file_matches_reference_program(tiny_models, tmp_path, wt):
    W.check_quantized_model_file_matches_reference_program(tiny_models, tmp_path, wt)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@both_types
@pytest.mark.parametrize("mode", ROWS[0].gpt2_modes)
def test_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode):
    W.check_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode)


@both_types
@pytest.mark.parametrize("B", ROWS[0].split_B)
def test_split_buffer_weights(rt, backend, wt, B):
    W.check_split_buffer_weights(rt, backend, wt, B)


def test_gguf_q2k_q3k_weights_on_mi355x(rt, backend, tmp_path):
    W.check_gguf_weights_on_mi355x(rt, backend, tmp_path, "q2k_q3k")
