"""GPU tests of IQ4_NL and IQ4_XS weights on the MI355X backend: GET_ROWS, MUL_MAT and MUL_MAT_ID in the
reference CPU's summation order (mmv_order=1: identical bits) and in tree order (mmv_order=0: within
1e-5 of the largest reference value), the default order of a quantized graph, a tiny GPT-2 of each
type end to end, split buffers and GGUF loading.

The reference is the reference CPU backend itself (oracle/_ref/libggml_ref.so, loaded isolated
beside the runtime) on identical inputs, or the committed fixtures tests/golden/iq4nl_*, iq4xs_*
where those suffice. The bodies that other types share are the check_* functions of
tests/weight_types.py, run on the table's IQ4_NL and IQ4_XS rows.
"""
import os

import numpy as np
import pytest

import weight_types as W
from ggml_mi355x import ggml as G
from weight_types import EXTREME_X, REF_GPT2, TREE_TOL, in_order, needs_ref, rel_err, same_bits
from weight_types import backend, ref, rt, tiny_models  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROWS = W.rows("iq4")
both_types = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)
CASES = [(wt, K, N) for wt in ROWS for K, N in wt.shapes]
CASE_IDS = [f"{wt.tag}-{K}x{N}" for wt, K, N in CASES]


@both_types
@pytest.mark.parametrize("which", ["w", "edge"])
def test_get_rows_matches_golden_dequantization(rt, backend, wt, which):
    W.check_get_rows_matches_golden_dequantization(rt, backend, wt, which)


@both_types
def test_mul_mat_matches_golden_output(rt, backend, wt):
    W.check_mul_mat_matches_golden_output(rt, backend, wt)


@needs_ref
@pytest.mark.parametrize("wt,K,N", CASES, ids=CASE_IDS)
def test_mul_mat_reference_order_bit_identical(rt, backend, wt, K, N):
    W.check_mul_mat_reference_order_bit_identical(rt, backend, wt, (K, N))


@needs_ref
@pytest.mark.parametrize("wt,K,N", CASES, ids=CASE_IDS)
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
def test_prequantized_src1(rt, backend, ref, wt, B):
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
def test_all_codes_rows_against_extreme_activations(rt, backend, ref, wt):
    """The edge fixture (its last row holds all sixteen codes in both nibble halves of every block)
    against the +-127 columns: pins the codebook lookup entry by entry, in both orders."""
    lib, cpu = ref
    T, K, N, B = wt.type, wt.manifest["edge"]["K"], wt.manifest["edge"]["N"], 2
    wq = wt.golden("edge.wq.bin")
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
@pytest.mark.parametrize("B", ROWS[0].chain_B)
def test_default_order_of_a_quantized_chain(rt, backend, ref, wt, B):
    W.check_default_order_of_a_quantized_chain(rt, backend, ref, wt, B)


@both_types
def test_supports_op_follows_the_table(rt, backend, wt):
    """MUL_MAT, MUL_MAT_ID and GET_ROWS are taken; an IQ4_NL row of an odd block count is refused
    (the reference's AVX2 dot walks the blocks in pairs and defines no result there)."""
    def supported(K):
        with G.Context(rt, rt.ggml_tensor_overhead() * 8, no_alloc=True) as c:
            w = rt.ggml_new_tensor_2d(c.ctx, wt.type, K, 4)
            x = rt.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, 2)
            i = rt.ggml_new_tensor_1d(c.ctx, G.GGML_TYPE_I32, 3)
            return (bool(rt.ggml_backend_supports_op(backend, rt.ggml_mul_mat(c.ctx, w, x))),
                    bool(rt.ggml_backend_supports_op(backend, rt.ggml_get_rows(c.ctx, w, i))))
    assert supported(256) == (True, True)
    if wt.tag == "iq4nl":
        assert supported(64) == (True, True) and supported(320) == (True, True)
        assert supported(32) == (False, True) and supported(96) == (False, True)


@needs_ref
@both_types
@pytest.mark.parametrize("n_tokens", ROWS[0].id_tokens)
def test_mul_mat_id_top2_of_4_experts(rt, backend, ref, wt, n_tokens):
    W.check_mul_mat_id_top2_of_4_experts(rt, backend, ref, wt, n_tokens)


@pytest.mark.skipif(not os.path.exists(REF_GPT2), reason="make -C oracle gpt2")
@both_types
@pytest.mark.parametrize("mode", ROWS[0].gpt2_modes)
def test_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode):
    W.check_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode)


@both_types
@pytest.mark.parametrize("B", ROWS[0].split_B)
def test_split_buffer_weights(rt, backend, wt, B):
    W.check_split_buffer_weights(rt, backend, wt, B)


def test_gguf_iq4_weights_on_mi355x(rt, backend, tmp_path):
    W.check_gguf_weights_on_mi355x(rt, backend, tmp_path, "iq4")
