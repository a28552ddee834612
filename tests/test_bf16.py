"""CPU tests of BF16 (GGML_TYPE_BF16 = 30) in the host runtime and the Python tables: the converters
against the reference library (oracle/_ref/libggml_ref.so, loaded isolated) over the converter's whole
input set, ggml_quantize_chunk, the model-file and GGUF paths, and the proof that the GPU tests' MUL_MAT
cases cannot pass vacuously: on their inputs each mutant of the reference's arithmetic changes an output bit.
"""
import struct

import numpy as np
import pytest

import bf16_cases as C
from conftest import golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import gguf
from ggml_mi355x import gpt2
from weight_types import TINY, ftype_to_type, needs_ref
from weight_types import ref as _ref_pair  # noqa: F401 (fixture)

BF16 = C.BF16


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def ref(_ref_pair):
    return _ref_pair[0]


def to_bf16_row(lib, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.size, np.uint16)
    lib.ggml_fp32_to_bf16_row(x.ctypes.data, out.ctypes.data, x.size)
    return out


def quantize_chunk(lib, x, K, start=0, out=None, nrows=None):
    x = np.ascontiguousarray(x, np.float32)
    n = x.size // K if nrows is None else nrows
    out = np.zeros(x.size, np.uint16) if out is None else out
    assert lib.ggml_quantize_chunk(BF16, x.ctypes.data, out.ctypes.data, start, n, K, None) == n * K * 2
    return out


# ------------------------------------------------------------------ fixtures and tables

def test_fixture_files_are_intact():
    m = C.manifest()
    assert set(m["files"]) == {"bf16_convert_sample.u16"} | set(m["cases"])
    for name, meta in m["files"].items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"] <= 24 * 1024, name
        assert C.sha256(blob) == meta["sha256"], name


def test_python_tables_know_bf16():
    assert G.GGML_TYPE_BF16 == 30 and G.TYPE_BY_NAME["bf16"] == 30
    assert G.BLOCK[30] == (1, 2)
    assert G.row_size(30, 1001) == 2002 and G.row_size(30, 4096) == 8192
    assert gpt2.FTYPES["bf16"] == (24, 30)


def test_type_traits(rt):
    assert rt.ggml_type_name(BF16) == b"bf16"
    assert rt.ggml_blck_size(BF16) == 1 and rt.ggml_type_size(BF16) == 2
    assert rt.ggml_row_size(BF16, 1001) == 2002
    assert not rt.ggml_is_quantized(BF16)
    assert ftype_to_type(rt, 24) == BF16


@needs_ref
def test_type_traits_match_reference(rt, ref):
    assert rt.ggml_type_name(BF16) == ref.ggml_type_name(BF16)
    assert rt.ggml_blck_size(BF16) == ref.ggml_blck_size(BF16) and rt.ggml_type_size(BF16) == ref.ggml_type_size(BF16)
    assert bool(rt.ggml_is_quantized(BF16)) == bool(ref.ggml_is_quantized(BF16))
    assert ftype_to_type(rt, 24) == ftype_to_type(ref, 24)


# ------------------------------------------------------------------ the converters

def test_converter_set_holds_every_class():
    u = C.converter_set()
    got = C.converter_classes(u)
    assert u.size == 393216 and len(np.unique(u)) == u.size
    assert got == C.manifest()["converter_set"]["classes"]
    # every class the reference converter treats on its own is there, in both signs where it has one
    assert got["pos_zero"] == 1 and got["neg_zero"] == 1
    assert got["subnormal"] == 2 * 128 * 6 - 2 and got["subnormal_neg"] == got["subnormal"] // 2
    assert got["tie_to_even_down"] == got["tie_to_even_up"] == 254 * 128
    assert got["below_half"] == got["above_half"] == 2 * 254 * 128
    assert got["carry_to_inf"] == 6  # +-0x7f7f8000, 0x7f7f8001, 0x7f7fffff
    assert got["inf"] == 2
    assert got["quiet_nan"] == 2 * 64 * 6 and got["signalling_nan"] == 2 * 64 * 6 - 2
    assert got["nan_payload_low_half_only"] == 10 and got["nan_payload_high_half_only"] == 2 * 127


def test_row_converter_matches_golden(rt):
    """The runtime's ggml_fp32_to_bf16_row over the whole set: the SHA-256 of the reference's outputs and its
    committed sample; the scalar function and the Python helper give the same bits."""
    u = C.converter_set()
    out = to_bf16_row(rt, u.view(np.float32))
    want = golden_blob("bf16_convert_sample.u16", np.uint16)
    idx = C.converter_sample(u)
    bad = np.flatnonzero(out[idx] != want)
    assert bad.size == 0, [(hex(u[idx[i]]), hex(out[idx[i]]), hex(want[i])) for i in bad[:8]]
    assert C.sha256(out) == C.manifest()["converter_set"]["sha256"]
    assert np.array_equal(G.f32_to_bf16(u.view(np.float32)), out)
    for i in idx[::97]:
        if (u[i] & 0x7fffffff) <= 0x7f800000:  # (a signalling NaN argument does not survive the call's float register)
            assert rt.ggml_fp32_to_bf16(float(u[i:i + 1].view(np.float32)[0])) == out[i], hex(u[i])


@needs_ref
def test_row_converter_matches_reference(rt, ref):
    x = C.converter_set().view(np.float32)
    out, want = to_bf16_row(rt, x), to_bf16_row(ref, x)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, [(hex(C.converter_set()[i]), hex(out[i]), hex(want[i])) for i in bad[:8]]


def test_bf16_to_f32_is_exact_for_every_pattern(rt):
    b = np.arange(65536, dtype=np.uint16)
    out = np.empty(65536, np.float32)
    rt.ggml_bf16_to_fp32_row(b.ctypes.data, out.ctypes.data, 65536)
    assert np.array_equal(out.view(np.uint32), b.astype(np.uint32) << 16)
    assert np.array_equal(G.bf16_to_f32(b).view(np.uint32), out.view(np.uint32))


@needs_ref
def test_bf16_to_f32_matches_reference(rt, ref):
    b = np.arange(65536, dtype=np.uint16)
    out, want = np.empty(65536, np.float32), np.empty(65536, np.float32)
    rt.ggml_bf16_to_fp32_row(b.ctypes.data, out.ctypes.data, 65536)
    ref.ggml_bf16_to_fp32_row(b.ctypes.data, want.ctypes.data, 65536)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_f16_to_bf16_over_every_f16_pattern(rt):
    """F16 -> f32 -> BF16, as the reference's CPY does it: the SHA-256 of the reference's outputs."""
    out = to_bf16_row(rt, C.f16_patterns_as_f32(rt))
    assert C.sha256(out) == C.manifest()["f16_to_bf16"]["sha256"]


@needs_ref
def test_f16_to_bf16_matches_reference(rt, ref):
    assert np.array_equal(to_bf16_row(rt, C.f16_patterns_as_f32(rt)), to_bf16_row(ref, C.f16_patterns_as_f32(ref)))


# ------------------------------------------------------------------ ggml_quantize_chunk

def test_quantize_chunk_bf16(rt):
    """The row conversion, rows of 32 and of an odd length; `start` places later rows where one call puts them."""
    x = C.converter_set().view(np.float32)
    want = G.f32_to_bf16(x)
    assert C.sha256(want) == C.manifest()["converter_set"]["sha256"]
    for K in (32, 3):
        assert np.array_equal(quantize_chunk(rt, x, K), want), K
    K, N = 96, x.size // 96
    out = np.zeros(x.size, np.uint16)
    quantize_chunk(rt, x, K, 0, out, nrows=5)
    assert np.array_equal(out[:5 * K], want[:5 * K]) and not out[5 * K:].any()
    quantize_chunk(rt, x, K, 5 * K, out, nrows=N - 5)
    assert np.array_equal(out, want)


@needs_ref
def test_quantize_chunk_matches_reference(rt, ref):
    x = C.converter_set().view(np.float32)
    K, N = 96, x.size // 96
    for lib_start in (0, 7 * K):
        a, b = np.zeros(x.size, np.uint16), np.zeros(x.size, np.uint16)
        quantize_chunk(rt, x, K, lib_start, a, nrows=N - lib_start // K)
        quantize_chunk(ref, x, K, lib_start, b, nrows=N - lib_start // K)
        assert np.array_equal(a, b), lib_start


# ------------------------------------------------------------------ the MUL_MAT cases are not vacuous

def test_cases_cover_every_axis_value():
    Ks, Ns, Bs = ({c[i] for c in C.CASES} for i in range(3))
    assert Ks >= {8, 32, 33, 40, 100, 256, 1000, 1001, 4096, 4104, 64, 320}
    assert Ns == {1, 5, 67} and Bs == {1, 2, 3, 5, 8, 9, 17, 33, 130}
    assert any(K == 1001 and B == 9 for K, _, B in C.CASES) and any(K == 4104 and B == 130 for K, _, B in C.CASES)
    assert {(N, B) for _, N, B in C.CASES} >= {(67, 33), (67, 130)}
    assert {(K, B) for K, _, B in C.CASES} >= {(64, 17), (320, 17)}
    for K, N, B in C.CASES:
        _, x = C.case_inputs(K, N, B)
        sub = x[:, C.SUBNORMAL_AT].view(np.uint32)
        assert ((sub & 0x7f800000) == 0).all() and ((sub & 0x7fffff) != 0).all()


def test_golden_outputs_match_the_numpy_restatement():
    """The committed reference outputs equal the numpy ggml_vec_dot_bf16, so the mutant test below stands
    on the reference's arithmetic even where its library is not built."""
    for name, c in C.manifest()["cases"].items():
        wb, x = C.case_inputs(c["K"], c["N"], c["B"])
        want = golden_blob(name, np.float32).reshape(c["B"], c["N"])
        assert np.array_equal(C.mul_mat_numpy(wb, x).view(np.uint32), want.view(np.uint32)), name


@pytest.mark.parametrize("K,N,B", C.CASES, ids=C.CASE_IDS)
def test_every_mutant_changes_an_output_bit(K, N, B):
    """Truncation instead of round-to-nearest-even, no subnormal flush, un-rounded f32 activations, a plain
    sequential f32 sum instead of the 4 x 8 lane order, f32 instead of double leftovers: each changes at
    least one output bit of every case whose K it applies to (bf16_cases.mutant_applies says where it
    cannot: the lane order needs a 32-step, f32 leftovers need two of them)."""
    wb, x = C.case_inputs(K, N, B)
    y = C.mul_mat_numpy(wb, x)
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    for m in C.MUTANTS:
        ym = C.mul_mat_numpy(wb, x, m)
        changed = not np.array_equal(ym.view(np.uint32), y.view(np.uint32))
        assert changed or not C.mutant_applies(m, K), (m, K)
    # every mutant is caught in every K class it applies to; each applies to at least six of the ten
    for m in C.MUTANTS:
        assert sum(C.mutant_applies(m, k) for k in (8, 32, 33, 40, 100, 256, 1000, 1001, 4096, 4104)) >= 6


@needs_ref
@pytest.mark.parametrize("K,N,B", C.CASES, ids=C.CASE_IDS)
def test_numpy_restatement_matches_reference_cpu(ref, _ref_pair, K, N, B):
    wb, x = C.case_inputs(K, N, B)
    yr = G.mul_mat_once(ref, _ref_pair[1], BF16, C.weight_bytes(wb), K, N, x.ravel(), B).reshape(B, N)
    assert np.array_equal(C.mul_mat_numpy(wb, x).view(np.uint32), yr.view(np.uint32))
    for m in C.MUTANTS:
        if C.mutant_applies(m, K):
            assert not np.array_equal(C.mul_mat_numpy(wb, x, m).view(np.uint32), yr.view(np.uint32)), m


# ------------------------------------------------------------------ model files

def test_quantize_model_bf16(rt, tmp_path):
    """quantize_model(..., "bf16"): ftype 24 (+ the quantization version), the 2-D weights as ttype 30 with
    ggml_quantize_chunk's bytes, everything else copied (test_bf16_gpu.py loads the file with the GPT-2 driver)."""
    f16 = gpt2.write_synthetic_model(str(tmp_path / "tiny-f16.bin"), **TINY)
    out = gpt2.quantize_model(rt, f16, str(tmp_path / "tiny-bf16.bin"), "bf16")

    def tensors(path):
        res = {}
        with open(path, "rb") as f:
            hdr = struct.unpack("7i", f.read(28))
            (nv,) = struct.unpack("i", f.read(4))
            for _ in range(nv):
                (ln,) = struct.unpack("i", f.read(4))
                f.read(ln)
            while True:
                head = f.read(12)
                if len(head) < 12:
                    break
                n_dims, name_len, ttype = struct.unpack("3i", head)
                ne = struct.unpack(f"{n_dims}i", f.read(4 * n_dims))
                name = f.read(name_len).decode()
                res[name] = (ttype, ne, f.read(int(np.prod(ne)) * (4 if ttype == 0 else 2)))
        return hdr, res

    h0, t0 = tensors(f16)
    h1, t1 = tensors(out)
    assert h1[:6] == h0[:6] and h1[6] == 24 + 2 * 1000
    assert list(t0) == list(t1)
    n_bf16 = 0
    for name, (ttype, ne, data) in t1.items():
        src_type, src_ne, src = t0[name]
        assert ne == src_ne
        if ttype == BF16:
            n_bf16 += 1
            f = np.frombuffer(src, np.float16 if src_type == 1 else np.float32).astype(np.float32)
            assert np.array_equal(np.frombuffer(data, np.uint16), G.f32_to_bf16(f)), name
        else:
            assert ttype == src_type and data == src, name
    import re
    named = [n for n, (_, ne, _d) in t0.items() if len(ne) == 2 and any(re.fullmatch(p, n) for p in gpt2.QUANT_TENSORS)]
    assert n_bf16 == len(named) >= 1 + 4 * TINY["n_layer"]


def test_gguf_carries_bf16_tensors(rt, tmp_path):
    """A BF16 tensor of an odd row length through the GGUF writer and reader: type, shape and bytes."""
    K, N = 33, 5
    wb, _ = C.case_inputs(33, 67, 3)
    data = C.weight_bytes(wb[:N])
    path = str(tmp_path / "bf16.gguf")
    gguf.write(rt, path, [("general.architecture", "str", "test")],
               [("pad", G.GGML_TYPE_F32, [3], np.zeros(3, np.float32)), ("w", BF16, [K, N], data)])
    params = G.gguf_init_params(no_alloc=True, ctx=None)
    g = rt.gguf_init_from_file(path.encode(), params)
    assert g
    try:
        i = rt.gguf_find_tensor(g, b"w")
        assert i >= 0 and rt.gguf_get_tensor_type(g, i) == BF16
        off = rt.gguf_get_data_offset(g) + rt.gguf_get_tensor_offset(g, i)
    finally:
        rt.gguf_free(g)
    with open(path, "rb") as f:
        f.seek(off)
        assert np.array_equal(np.frombuffer(f.read(data.size), np.uint8), data)
