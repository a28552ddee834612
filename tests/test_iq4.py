"""CPU tests of the IQ4_NL / IQ4_XS host side (no GPU): ggml_quantize_chunk writes the reference's
bytes -- against the committed fixtures (tests/golden/iq4nl_*, iq4xs_*, written by
tests/golden/make_iq4_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref). The bodies that other types share are the check_*
functions of tests/weight_types.py, run on the table's IQ4_NL and IQ4_XS rows."""
import numpy as np
import pytest

import weight_types as W
from ggml_mi355x import ggml as G
from weight_types import REF_LIB, needs_ref, quantize
from weight_types import rt  # noqa: F401 (fixture)

ROWS = W.rows("iq4")
by_tag = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def test_fixture_files_are_intact():
    W.check_fixture_files_are_intact("iq4")


def test_python_tables_know_the_types():
    W.check_python_tables_know_the_types("iq4")


@by_tag
def test_type_traits(rt, wt):
    W.check_type_traits(rt, wt)


@needs_ref
@by_tag
def test_type_traits_match_reference(rt, ref, wt):
    W.check_type_traits_match_reference(rt, ref, wt)


@pytest.mark.parametrize("ftype,t", [(19, 20), (22, 23)])
def test_ftype_to_type(rt, ftype, t):
    assert rt.ggml_ftype_to_ggml_type(ftype) == t


@needs_ref
@pytest.mark.parametrize("ftype", [19, 22])
def test_ftype_to_type_matches_reference(rt, ref, ftype):
    assert rt.ggml_ftype_to_ggml_type(ftype) == ref.ggml_ftype_to_ggml_type(ftype)


@pytest.mark.parametrize("which", ["w", "edge"])
@by_tag
def test_quantize_chunk_matches_golden_bytes(rt, wt, which):
    W.check_quantize_chunk_matches_golden_bytes(rt, wt, which)


@by_tag
def test_quantize_chunk_start_offset(rt, wt):
    W.check_quantize_chunk_start_offset(rt, wt)


def test_all_zero_input_bytes(rt):
    """IQ4: zero input is not zero bytes: index 8 (the level 1) is the nearest to 0, and IQ4_XS's
    d = -max_scale / 32 is fp16 -0.0 with every 6-bit scale 32 (scales_h 0xAAAA, scales_l 0)."""
    nl = quantize(rt, 20, np.zeros(64, np.float32), 64).reshape(2, 18)
    assert (nl[:, 0:2] == 0).all() and (nl[:, 2:] == 0x88).all()
    xs = quantize(rt, 23, np.zeros(512, np.float32), 512).reshape(2, 136)
    assert (xs[:, 0] == 0x00).all() and (xs[:, 1] == 0x80).all()
    assert (xs[:, 2:4] == 0xAA).all() and (xs[:, 4:8] == 0).all() and (xs[:, 8:] == 0x88).all()


@by_tag
def test_codebook_row_uses_all_sixteen_codes(wt):
    """The last edge row (kvalues and its reverse times 0.01, tiled): every code in both nibble halves."""
    N = wt.manifest["edge"]["N"]
    row = wt.golden("edge.wq.bin").reshape(N, -1)[N - 1].reshape(-1, wt.block_bytes)
    qs = row[:, wt.fields["qs"]]
    assert set((qs & 15).ravel().tolist()) == set(range(16)) and set((qs >> 4).ravel().tolist()) == set(range(16))


@needs_ref
@pytest.mark.parametrize("K", ROWS[0].quant_K)
@by_tag
def test_quantize_chunk_matches_reference(rt, ref, wt, K):
    W.check_quantize_chunk_matches_reference(rt, ref, wt, K)
