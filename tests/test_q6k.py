"""CPU tests of the Q6_K host side (no GPU): ggml_quantize_chunk(GGML_TYPE_Q6_K) writes the
reference's bytes -- against the committed fixtures (tests/golden/q6k_*, written by
tests/golden/make_q6k_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref). The bodies are the check_* functions of
tests/weight_types.py, run on the table's Q6_K row."""
import pytest

import weight_types as W
from ggml_mi355x import ggml as G
from weight_types import REF_LIB, needs_ref
from weight_types import rt  # noqa: F401 (fixture)

WT, = W.rows("q6k")


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def test_fixture_files_are_intact():
    W.check_fixture_files_are_intact("q6k")


def test_python_tables_know_q6k():
    W.check_python_tables_know_the_types("q6k")


def test_type_traits(rt):
    W.check_type_traits(rt, WT)


@needs_ref
def test_type_traits_match_reference(rt, ref):
    W.check_type_traits_match_reference(rt, ref, WT)


@pytest.mark.parametrize("which", ["w", "edge"])
def test_quantize_chunk_matches_golden_bytes(rt, which):
    W.check_quantize_chunk_matches_golden_bytes(rt, WT, which)


def test_quantize_chunk_start_offset(rt):
    W.check_quantize_chunk_start_offset(rt, WT)


def test_all_zero_superblock_is_all_zero_bytes(rt):
    W.check_all_zero_input_is_all_zero_bytes(rt, WT)


@needs_ref
@pytest.mark.parametrize("K", WT.quant_K)
def test_quantize_chunk_matches_reference(rt, ref, K):
    W.check_quantize_chunk_matches_reference(rt, ref, WT, K)
