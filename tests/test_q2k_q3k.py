"""CPU tests of the Q2_K / Q3_K host side (no GPU): ggml_quantize_chunk writes the reference's
bytes -- against the committed fixtures (tests/golden/q2k_*, q3k_*, written by
tests/golden/make_q2k_q3k_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref). The bodies are the check_* functions of
tests/weight_types.py, run on the table's Q2_K and Q3_K rows."""
import pytest

import weight_types as W
from ggml_mi355x import ggml as G
from weight_types import REF_LIB, needs_ref
from weight_types import rt  # noqa: F401 (fixture)

ROWS = W.rows("q2k_q3k")
by_tag = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def test_fixture_files_are_intact():
    W.check_fixture_files_are_intact("q2k_q3k")


def test_python_tables_know_the_types():
    W.check_python_tables_know_the_types("q2k_q3k")


@by_tag
def test_type_traits(rt, wt):
    W.check_type_traits(rt, wt)


@needs_ref
@by_tag
def test_type_traits_match_reference(rt, ref, wt):
    W.check_type_traits_match_reference(rt, ref, wt)


@pytest.mark.parametrize("which", ["w", "edge"])
@by_tag
def test_quantize_chunk_matches_golden_bytes(rt, wt, which):
    W.check_quantize_chunk_matches_golden_bytes(rt, wt, which)


@by_tag
def test_quantize_chunk_start_offset(rt, wt):
    W.check_quantize_chunk_start_offset(rt, wt)


@by_tag
def test_all_zero_input_is_all_zero_bytes(rt, wt):
    W.check_all_zero_input_is_all_zero_bytes(rt, wt)


@needs_ref
@pytest.mark.parametrize("K", ROWS[0].quant_K)
@by_tag
def test_quantize_chunk_matches_reference(rt, ref, wt, K):
    W.check_quantize_chunk_matches_reference(rt, ref, wt, K)
