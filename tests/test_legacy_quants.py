"""CPU tests of the Q4_1 / Q5_0 / Q5_1 host side (no GPU): ggml_quantize_chunk writes the
reference's bytes -- against the committed fixtures (tests/golden/legacy_*, written by
tests/golden/make_legacy_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref); the block layouts of the fixtures dequantize to the
reference's floats; gpt2.quantize_model writes the reference quantize program's files."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import gpt2 as gpt2mod
from ggml_mi355x import synth

REF = os.path.join(REPO, "oracle", "_ref")
REF_LIB = os.path.join(REF, "libggml_ref.so")
REF_QUANTIZE = os.path.join(REF, "gpt-2-quantize")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference build (oracle/_ref) absent")
# (the quantizers' roundings are written out with fmaf, so an instrumented build of the host runtime
# -- GGML_MI355X_CORE_LIB, as tests/test_core.py -- writes the same bytes: nothing is skipped for it)
TYPES = {"q4_1": 3, "q5_0": 6, "q5_1": 7}
BLOCK_BYTES = {3: 20, 6: 22, 7: 24}
FTYPE = {"q4_1": 3, "q5_0": 8, "q5_1": 9}
Q8_0, Q8_1 = 8, 9
NAMES = sorted(TYPES)

with open(os.path.join(GOLDEN, "legacy.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def ftype_to_type(lib, ftype):
    for h in lib.handles:
        if hasattr(h, "ggml_ftype_to_ggml_type"):
            return int(h.ggml_ftype_to_ggml_type(ftype))
    raise AssertionError("ggml_ftype_to_ggml_type is not exported")


def quantize(lib, t, w, K):
    w = np.ascontiguousarray(w, np.float32)
    n = w.size // K
    out = np.empty(G.row_size(t, K) * n, np.uint8)
    assert lib.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
    return out


def fields(t):
    if t == 3:
        return {"d": slice(0, 2), "m": slice(2, 4), "qs": slice(4, 20)}
    if t == 6:
        return {"d": slice(0, 2), "qh": slice(2, 6), "qs": slice(6, 22)}
    return {"d": slice(0, 2), "m": slice(2, 4), "qh": slice(4, 8), "qs": slice(8, 24)}


def describe(t, out, want):
    """Which blocks / fields differ (for the assertion message)."""
    a, b = out.reshape(-1, BLOCK_BYTES[t]), want.reshape(-1, BLOCK_BYTES[t])
    bad = np.flatnonzero((a != b).any(axis=1))
    what = {k: int((a[bad][:, s] != b[bad][:, s]).sum()) for k, s in fields(t).items()}
    return f"{bad.size} of {a.shape[0]} blocks differ (first {bad[:4].tolist()}): bytes per field {what}"


def dequantize(t, blocks):
    """The block layouts in numpy, each value with the reference's f32 operations: Q4_1 / Q5_1
    q * d + m, Q5_0 (q - 16) * d; element j < 16 from the low nibble of qs[j], j >= 16 from the high
    nibble of qs[j - 16], bit j of the little-endian qh its fifth bit."""
    b = blocks.reshape(-1, BLOCK_BYTES[t])
    f = fields(t)
    d = b[:, f["d"]].copy().view(np.float16).astype(np.float32)
    qs = b[:, f["qs"]]
    q = np.concatenate([qs & 0x0F, qs >> 4], axis=1).astype(np.int32)
    if "qh" in f:
        qh = b[:, f["qh"]].copy().view("<u4")
        q |= (((qh >> np.arange(32, dtype=np.uint32)) & 1) << 4).astype(np.int32)
    if t == 6:
        return ((q - 16).astype(np.float32) * d).ravel()
    m = b[:, f["m"]].copy().view(np.float16).astype(np.float32)
    return (q.astype(np.float32) * d + m).astype(np.float32).ravel()


def test_fixture_files_are_intact():
    for name, meta in MANIFEST["files"].items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"], name
        assert hashlib.sha256(blob.tobytes()).hexdigest() == meta["sha256"], name


def test_python_tables_know_the_types():
    assert (G.GGML_TYPE_Q4_1, G.GGML_TYPE_Q5_0, G.GGML_TYPE_Q5_1, G.GGML_TYPE_Q8_1) == (3, 6, 7, 9)
    for name, t in TYPES.items():
        assert G.TYPE_BY_NAME[name] == t and G.BLOCK[t] == (32, BLOCK_BYTES[t])
        assert G.row_size(t, 11008) == 344 * BLOCK_BYTES[t]
        assert gpt2mod.FTYPES[name] == (FTYPE[name], t)
    assert G.BLOCK[Q8_1] == (32, 36)


@pytest.mark.parametrize("name", NAMES)
def test_type_traits(rt, name):
    t = TYPES[name]
    assert rt.ggml_type_name(t) == name.encode()
    assert rt.ggml_blck_size(t) == 32 and rt.ggml_type_size(t) == BLOCK_BYTES[t]
    for K in (32, 96, 4096, 11008):
        assert rt.ggml_row_size(t, K) == K // 32 * BLOCK_BYTES[t]
    assert ftype_to_type(rt, FTYPE[name]) == t
    assert rt.ggml_type_size(Q8_1) == 36 and rt.ggml_blck_size(Q8_1) == 32


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_type_traits_match_reference(rt, ref, name):
    t = TYPES[name]
    assert rt.ggml_type_name(t) == ref.ggml_type_name(t)
    assert rt.ggml_blck_size(t) == ref.ggml_blck_size(t)
    assert rt.ggml_type_size(t) == ref.ggml_type_size(t)
    for K in (32, 800, 11008):
        assert rt.ggml_row_size(t, K) == ref.ggml_row_size(t, K)
    assert ftype_to_type(rt, FTYPE[name]) == ftype_to_type(ref, FTYPE[name])


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_vec_dot_type_is_the_reference_s(ref, name):
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
    tr = f(TYPES[name])
    assert tr.type_name == name.encode() and tr.type_size == BLOCK_BYTES[TYPES[name]]
    assert tr.vec_dot_type == (Q8_0 if name == "q5_0" else Q8_1)


@pytest.mark.parametrize("which", ["w", "edge"])
@pytest.mark.parametrize("name", NAMES)
def test_quantize_chunk_matches_golden_bytes(rt, name, which):
    t, K = TYPES[name], MANIFEST[which]["K"]
    out = quantize(rt, t, golden_blob(f"legacy_{which}.f32", np.float32), K)
    want = golden_blob(f"legacy_{name}_{which}.wq.bin")
    assert np.array_equal(out, want), describe(t, out, want)


@pytest.mark.parametrize("which", ["w", "edge"])
@pytest.mark.parametrize("name", NAMES)
def test_dequantization_matches_golden_bits(name, which):
    """The block layout as this project reads it (GET_ROWS, the GEMV kernels) gives dequantize_row_*'s bits."""
    t = TYPES[name]
    got = dequantize(t, golden_blob(f"legacy_{name}_{which}.wq.bin"))
    want = golden_blob(f"legacy_{name}_{which}.wdq.f32", np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())


@pytest.mark.parametrize("name", NAMES)
def test_quantize_chunk_start_offset(rt, name):
    """Rows quantized in two calls (start = 0 and start = 3 rows) land where one call puts them."""
    t, K, N = TYPES[name], MANIFEST["w"]["K"], MANIFEST["w"]["N"]
    w = golden_blob("legacy_w.f32", np.float32)
    rs = G.row_size(t, K)
    out = np.zeros(rs * N, np.uint8)
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, 3, K, None) == 3 * rs
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 3 * K, N - 3, K, None) == (N - 3) * rs
    assert np.array_equal(out, quantize(rt, t, w, K))


@pytest.mark.parametrize("name", NAMES)
def test_all_zero_block(rt, name):
    """d = 0 and m = 0; the levels are the reference's: 0 for Q4_1 / Q5_1, 16 (bit 4 set, nibble 0) for
    Q5_0, whose d = 0 / -16 is the fp16 negative zero."""
    t = TYPES[name]
    out = quantize(rt, t, np.zeros(64, np.float32), 64).reshape(2, -1)
    f = fields(t)
    assert not out[:, f["qs"]].any()
    if t == 6:
        assert (out[:, f["qh"]] == 0xFF).all() and (out[:, f["d"]] == [0x00, 0x80]).all()
    else:
        assert not out.any()


def _edge_rows(K):
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)
    r = synth.uniform(44, K).copy(); r[3] = -2.0; r[9] = 2.0; rows.append(r)              # +a and -a both largest
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # fp16-subnormal / zero d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)                   # d near the fp16 range
    r = np.abs(synth.uniform(48, K)) + 3.0; rows.append(r.astype(np.float32))             # large positive min
    return np.stack(rows)


@needs_ref
@pytest.mark.parametrize("K", [32, 96, 4096])
@pytest.mark.parametrize("name", NAMES)
def test_quantize_chunk_matches_reference(rt, ref, name, K):
    """Some thousand random blocks (plain and widely scaled) and the edge rows: the reference's bytes."""
    t = TYPES[name]
    rng = np.random.default_rng(1000 + K + t)
    n = max(4, 65536 // K)
    w = np.concatenate([rng.standard_normal(n * K).astype(np.float32),
                        (rng.standard_normal(n * K) * rng.uniform(1e-3, 30.0, n * K)).astype(np.float32),
                        _edge_rows(K).ravel()])
    out, want = quantize(rt, t, w, K), quantize(ref, t, w, K)
    assert out.size // BLOCK_BYTES[t] >= 4096
    assert np.array_equal(out, want), describe(t, out, want)


def test_importance_matrices_stay_refused():
    """ggml_quantize_chunk with an imatrix aborts for these types (a child process: it is an assert)."""
    code = ("import numpy as np\nfrom ggml_mi355x import ggml as G\nrt = G.runtime()\n"
            "w = np.ones(32, np.float32); o = np.empty(64, np.uint8)\n"
            "rt.ggml_quantize_chunk(3, w.ctypes.data, o.ctypes.data, 0, 1, 32, w.ctypes.data)\nprint('survived')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "ggml-imax_amd"))
    p = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode != 0 and "survived" not in p.stdout
    assert "importance-matrix" in p.stderr


TINY = dict(n_embd=64, n_head=2, n_layer=1, n_vocab=96, n_ctx=16)


@pytest.mark.skipif(not os.path.exists(REF_QUANTIZE), reason="make -C oracle gpt2")
@pytest.mark.parametrize("name", NAMES)
def test_quantized_model_file_matches_reference_program(rt, tmp_path, name):
    import filecmp
    f16 = gpt2mod.write_synthetic_model(str(tmp_path / "tiny-f16.bin"), **TINY)
    ours = gpt2mod.quantize_model(rt, f16, str(tmp_path / f"tiny-{name}.bin"), name)
    out = str(tmp_path / f"ref-{name}.bin")
    p = subprocess.run([REF_QUANTIZE, f16, out, name], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(ours) == os.path.getsize(out)
    assert filecmp.cmp(ours, out, shallow=False)
