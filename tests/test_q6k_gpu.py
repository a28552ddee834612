"""GPU tests of Q6_K weights on the MI355X backend: GET_ROWS, MUL_MAT in the reference CPU's
summation order (mmv_order=1: identical bits) and in tree order (mmv_order=0: within 1e-5), the
default order of a quantized graph, a tiny Q6_K GPT-2 end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/q6k_* where those
suffice. The bodies are the check_* functions of tests/weight_types.py, run on the table's Q6_K row.
"""
import os

import pytest

import weight_types as W
from weight_types import REF_GPT2, REF_QUANTIZE, needs_ref
from weight_types import backend, ref, rt, tiny_models  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

WT, = W.rows("q6k")


@pytest.mark.parametrize("which", ["w", "edge"])
def test_get_rows_matches_golden_dequantization(rt, backend, which):
    W.check_get_rows_matches_golden_dequantization(rt, backend, WT, which)


def test_mul_mat_matches_golden_output(rt, backend):
    W.check_mul_mat_matches_golden_output(rt, backend, WT)


@needs_ref
@pytest.mark.parametrize("K,N", WT.shapes)
def test_mul_mat_reference_order_bit_identical(rt, backend, K, N):
    W.check_mul_mat_reference_order_bit_identical(rt, backend, WT, (K, N))


@needs_ref
@pytest.mark.parametrize("K,N", WT.shapes)
def test_mul_mat_tree_order(rt, backend, K, N):
    W.check_mul_mat_tree_order(rt, backend, WT, (K, N))


@needs_ref
def test_mul_mat_llama_ffn_down_rows(rt, backend, ref):
    W.check_mul_mat_llama_ffn_down_rows(rt, backend, ref, WT)


@needs_ref
@pytest.mark.parametrize("ne11", [1, 3, 9])
def test_weight_batch_and_strided_src1(rt, backend, ref, ne11):
    W.check_weight_batch_and_strided_src1(rt, backend, ref, WT, ne11)


@needs_ref
@pytest.mark.parametrize("B", WT.prequant_B)
def test_prequantized_q8k_src1(rt, backend, ref, B):
    W.check_prequantized_src1(rt, backend, ref, WT, B)


@needs_ref
def test_three_independent_mul_mats_in_one_graph(rt, backend, ref):
    W.check_three_independent_mul_mats_in_one_graph(rt, backend, ref, WT)


@needs_ref
def test_extreme_integers(rt, backend, ref):
    W.check_extreme_integers(rt, backend, ref, WT)


@needs_ref
@pytest.mark.parametrize("B", WT.chain_B)
def test_default_order_of_a_quantized_chain(rt, backend, ref, B):
    W.check_default_order_of_a_quantized_chain(rt, backend, ref, WT, B)


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
def test_quantized_model_file_matches_reference_program(tiny_models, tmp_path):
    W.check_quantized_model_file_matches_reference_program(tiny_models, tmp_path, WT)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@pytest.mark.parametrize("mode", WT.gpt2_modes)
def test_gpt2_q6k_logits_bit_identical_to_reference_cpu(tiny_models, mode):
    W.check_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, WT, mode)


@pytest.mark.parametrize("B", WT.split_B)
def test_split_buffer_weights(rt, backend, B):
    W.check_split_buffer_weights(rt, backend, WT, B)


def test_gguf_q6k_weights_on_mi355x(rt, backend, tmp_path):
    W.check_gguf_weights_on_mi355x(rt, backend, tmp_path, "q6k")
