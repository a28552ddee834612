"""CPU tests of the Q4_1 / Q5_0 / Q5_1 host side (no GPU): ggml_quantize_chunk writes the
reference's bytes -- against the committed fixtures (tests/golden/legacy_*, written by
tests/golden/make_legacy_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref); the block layouts of the fixtures dequantize to the
reference's floats; gpt2.quantize_model writes the reference quantize program's files. The bodies
that other types share are the check_* functions of tests/weight_types.py, run on the table's
Q4_1, Q5_0 and Q5_1 rows."""
import os
import subprocess

import numpy as np
import pytest

import weight_types as W
from conftest import REPO
from ggml_mi355x import ggml as G
from ggml_mi355x import gpt2 as gpt2mod
from weight_types import REF_LIB, REF_QUANTIZE, needs_ref, quantize
from weight_types import rt  # noqa: F401 (fixture)

# (the quantizers' roundings are written out with fmaf, so an instrumented build of the host runtime
# -- GGML_MI355X_CORE_LIB, as tests/test_core.py -- writes the same bytes: nothing is skipped for it)
ROWS = W.rows("legacy")
by_name = pytest.mark.parametrize("wt", ROWS, ids=lambda wt: wt.tag)


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def dequantize(wt, blocks):
    """The 32-element block layouts in numpy, each value with the reference's f32 operations: Q4_1 /
    Q5_1 q * d + m, Q5_0 (q - 16) * d; element j < 16 from the low nibble of qs[j], j >= 16 from the
    high nibble of qs[j - 16], bit j of the little-endian qh its fifth bit."""
    b = blocks.reshape(-1, wt.block_bytes)
    f = wt.fields
    d = b[:, f["d"]].copy().view(np.float16).astype(np.float32)
    qs = b[:, f["qs"]]
    q = np.concatenate([qs & 0x0F, qs >> 4], axis=1).astype(np.int32)
    if "qh" in f:
        qh = b[:, f["qh"]].copy().view("<u4")
        q |= (((qh >> np.arange(32, dtype=np.uint32)) & 1) << 4).astype(np.int32)
    if "m" not in f:
        return ((q - 16).astype(np.float32) * d).ravel()
    m = b[:, f["m"]].copy().view(np.float16).astype(np.float32)
    return (q.astype(np.float32) * d + m).astype(np.float32).ravel()


def test_fixture_files_are_intact():
    W.check_fixture_files_are_intact("legacy")


def test_python_tables_know_the_types():
    W.check_python_tables_know_the_types("legacy")


@by_name
def test_type_traits(rt, wt):
    W.check_type_traits(rt, wt)


@needs_ref
@by_name
def test_type_traits_match_reference(rt, ref, wt):
    W.check_type_traits_match_reference(rt, ref, wt)


@needs_ref
@by_name
def test_vec_dot_type_is_the_reference_s(ref, wt):
    """The activation format the backend quantizes src1 to (Q5_0: Q8_0; Q4_1 / Q5_1: Q8_1) is the
    reference's vec_dot_type: the committed reference mul_mat output is reproduced from the fixture
    blocks only with it (tests/test_legacy_quants_gpu.py); here the reference's own table is read."""
    import ctypes

    class Traits(ctypes.Structure):
        _fields_ = [("type_name", ctypes.c_char_p), ("blck_size", ctypes.c_int), ("type_size", ctypes.c_size_t),
                    ("is_quantized", ctypes.c_bool), ("to_float", ctypes.c_void_p), ("from_float", ctypes.c_void_p),
                    ("from_float_reference", ctypes.c_void_p), ("vec_dot", ctypes.c_void_p), ("vec_dot_type", ctypes.c_int),
                    ("nrows", ctypes.c_int64)]

    f = ref.handles[0].ggml_internal_get_type_traits
    f.restype = Traits
    f.argtypes = [ctypes.c_int]
    tr = f(wt.type)
    assert tr.type_name == wt.name.encode() and tr.type_size == wt.block_bytes
    assert tr.vec_dot_type == wt.act


@pytest.mark.parametrize("which", ["w", "edge"])
@by_name
def test_quantize_chunk_matches_golden_bytes(rt, wt, which):
    W.check_quantize_chunk_matches_golden_bytes(rt, wt, which)


@pytest.mark.parametrize("which", ["w", "edge"])
@by_name
def test_dequantization_matches_golden_bits(wt, which):
    """The block layout as this project reads it (GET_ROWS, the GEMV kernels) gives dequantize_row_*'s bits."""
    got = dequantize(wt, wt.golden(f"{which}.wq.bin"))
    want = wt.golden(f"{which}.wdq.f32", np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())


@by_name
def test_quantize_chunk_start_offset(rt, wt):
    W.check_quantize_chunk_start_offset(rt, wt)


@by_name
def test_all_zero_block(rt, wt):
    """d = 0 and m = 0; the levels are the reference's: 0 for Q4_1 / Q5_1, 16 (bit 4 set, nibble 0) for
    Q5_0, whose d = 0 / -16 is the fp16 negative zero."""
    out = quantize(rt, wt.type, np.zeros(64, np.float32), 64).reshape(2, -1)
    f = wt.fields
    assert not out[:, f["qs"]].any()
    if wt.tag == "q5_0":
        assert (out[:, f["qh"]] == 0xFF).all() and (out[:, f["d"]] == [0x00, 0x80]).all()
    else:
        assert not out.any()


@needs_ref
@pytest.mark.parametrize("K", ROWS[0].quant_K)
@by_name
def test_quantize_chunk_matches_reference(rt, ref, wt, K):
    W.check_quantize_chunk_matches_reference(rt, ref, wt, K)


def test_importance_matrices_stay_refused():
    """ggml_quantize_chunk with an imatrix aborts for the 32-element types (a child process: it is an assert)."""
    code = ("import numpy as np\nfrom ggml_mi355x import ggml as G\nrt = G.runtime()\n"
            "w = np.ones(32, np.float32); o = np.empty(64, np.uint8)\n"
            "rt.ggml_quantize_chunk(3, w.ctypes.data, o.ctypes.data, 0, 1, 32, w.ctypes.data)\nprint('survived')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "ggml-imax_amd"))
    p = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode != 0 and "survived" not in p.stdout
    assert "importance-matrix" in p.stderr


TINY = dict(n_embd=64, n_head=2, n_layer=1, n_vocab=96, n_ctx=16)


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
@by_name
def test_quantized_model_file_matches_reference_program(rt, tmp_path, wt):
    import filecmp
    f16 = gpt2mod.write_synthetic_model(str(tmp_path / "tiny-f16.bin"), **TINY)
    ours = gpt2mod.quantize_model(rt, f16, str(tmp_path / f"tiny-{wt.model}.bin"), wt.model)
    out = str(tmp_path / f"ref-{wt.model}.bin")
    p = subprocess.run([REF_QUANTIZE, f16, out, wt.model], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(ours) == os.path.getsize(out)
    assert filecmp.cmp(ours, out, shallow=False)
