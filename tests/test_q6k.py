"""CPU tests of the Q6_K host side (no GPU): ggml_quantize_chunk(GGML_TYPE_Q6_K) writes the
reference's bytes -- against the committed fixtures (tests/golden/q6k_*, written by
tests/golden/make_q6k_golden.py from the reference build) everywhere, and against the reference
libggml itself where it is built (oracle/_ref)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import gpt2 as gpt2mod
from ggml_mi355x import synth

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference build (oracle/_ref) absent")
# an instrumented build of the host runtime: the quantizers' bytes follow gcc's FMA contraction
# of the release flags, which instrumentation can change (as tests/test_core.py)
INSTRUMENTED = bool(os.environ.get("GGML_MI355X_CORE_LIB"))
Q6_K = 14

with open(os.path.join(GOLDEN, "q6k.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def quantize(lib, w, K):
    w = np.ascontiguousarray(w, np.float32)
    n = w.size // K
    out = np.empty(G.row_size(Q6_K, K) * n, np.uint8)
    assert lib.ggml_quantize_chunk(Q6_K, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
    return out


def describe(out, want, K):
    """Which blocks / fields differ (for the assertion message)."""
    a, b = out.reshape(-1, 210), want.reshape(-1, 210)
    bad = np.flatnonzero((a != b).any(axis=1))
    fields = {"ql": slice(0, 128), "qh": slice(128, 192), "scales": slice(192, 208), "d": slice(208, 210)}
    what = {k: int((a[bad][:, s] != b[bad][:, s]).sum()) for k, s in fields.items()}
    return f"{bad.size} of {a.shape[0]} blocks differ (first {bad[:4].tolist()}, K={K}): bytes per field {what}"


def test_fixture_files_are_intact():
    for name, meta in MANIFEST["files"].items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"], name
        assert hashlib.sha256(blob.tobytes()).hexdigest() == meta["sha256"], name


def test_python_tables_know_q6k():
    assert G.GGML_TYPE_Q6_K == Q6_K and G.TYPE_BY_NAME["q6_K"] == Q6_K and G.BLOCK[Q6_K] == (256, 210)
    assert G.row_size(Q6_K, 11008) == 43 * 210
    assert gpt2mod.FTYPES["q6_k"] == (14, Q6_K)


def test_type_traits(rt):
    assert rt.ggml_type_name(Q6_K) == b"q6_K"
    assert rt.ggml_blck_size(Q6_K) == 256 and rt.ggml_type_size(Q6_K) == 210
    for K in (256, 768, 4096, 11008):
        assert rt.ggml_row_size(Q6_K, K) == K // 256 * 210


@needs_ref
def test_type_traits_match_reference(rt, ref):
    assert rt.ggml_type_name(Q6_K) == ref.ggml_type_name(Q6_K)
    assert rt.ggml_blck_size(Q6_K) == ref.ggml_blck_size(Q6_K)
    assert rt.ggml_type_size(Q6_K) == ref.ggml_type_size(Q6_K)
    for K in (256, 2816, 11008):
        assert rt.ggml_row_size(Q6_K, K) == ref.ggml_row_size(Q6_K, K)


@pytest.mark.parametrize("which", ["w", "edge"])
def test_quantize_chunk_matches_golden_bytes(rt, which):
    K = MANIFEST[which]["K"]
    out = quantize(rt, golden_blob(f"q6k_{which}.f32", np.float32), K)
    if INSTRUMENTED:
        return
    want = golden_blob(f"q6k_{which}.wq.bin")
    assert np.array_equal(out, want), describe(out, want, K)


def test_quantize_chunk_start_offset(rt):
    """Rows quantized in two calls (start = 0 and start = 3 rows) land where one call puts them."""
    K, N = MANIFEST["w"]["K"], MANIFEST["w"]["N"]
    w = golden_blob("q6k_w.f32", np.float32)
    out = np.zeros(G.row_size(Q6_K, K) * N, np.uint8)
    rs = G.row_size(Q6_K, K)
    assert rt.ggml_quantize_chunk(Q6_K, w.ctypes.data, out.ctypes.data, 0, 3, K, None) == 3 * rs
    assert rt.ggml_quantize_chunk(Q6_K, w.ctypes.data, out.ctypes.data, 3 * K, N - 3, K, None) == (N - 3) * rs
    assert np.array_equal(out, quantize(rt, w, K))


def test_all_zero_superblock_is_all_zero_bytes(rt):
    out = quantize(rt, np.zeros(512, np.float32), 512)
    assert not out.any()


def _edge_rows(K):
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)      # negative largest scale
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)     # positive largest scale
    r = synth.uniform(44, K).copy(); r[32:48] = 0.0; rows.append(r)                       # one zero sub-block
    r = synth.uniform(45, K).copy(); r[:256] = 0.0; rows.append(r)                        # zero superblock first
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # fp16-subnormal / zero d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)
    return np.stack(rows)


@needs_ref
@pytest.mark.parametrize("K", [256, 768, 2816])
def test_quantize_chunk_matches_reference(rt, ref, K):
    if INSTRUMENTED:
        pytest.skip("instrumented host build: bytes follow the release flags' FMA contraction")
    rng = np.random.default_rng(1000 + K)
    n = max(4, 16384 // K)
    w = np.concatenate([rng.standard_normal(n * K).astype(np.float32),
                        (rng.standard_normal(4 * K) * rng.uniform(1e-3, 30.0, 4 * K)).astype(np.float32),
                        _edge_rows(K).ravel()])
    out, want = quantize(rt, w, K), quantize(ref, w, K)
    assert np.array_equal(out, want), describe(out, want, K)
