"""CPU tests of the Q2_K / Q3_K host side (no GPU): ggml_quantize_chunk writes the reference's
bytes -- against the committed fixtures (tests/golden/q2k_*, q3k_*, written by
tests/golden/make_q2k_q3k_golden.py from the reference build) everywhere, and against the reference
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
Q2_K, Q3_K = 10, 11
# tag, ggml type, name, block bytes, the block's fields
TYPES = {
    "q2k": (Q2_K, b"q2_K", 84, {"scales": slice(0, 16), "qs": slice(16, 80), "d": slice(80, 82), "dmin": slice(82, 84)}),
    "q3k": (Q3_K, b"q3_K", 110, {"hmask": slice(0, 32), "qs": slice(32, 96), "scales": slice(96, 108), "d": slice(108, 110)}),
}
TAGS = list(TYPES)

with open(os.path.join(GOLDEN, "q2k_q3k.json")) as _f:
    MANIFEST = json.load(_f)


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    G.Context(lib, 1024).free()  # the reference fills its tables in the first ggml_init
    return lib


def quantize(lib, t, w, K):
    w = np.ascontiguousarray(w, np.float32)
    n = w.size // K
    out = np.empty(G.row_size(t, K) * n, np.uint8)
    assert lib.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
    return out


def describe(tag, out, want, K):
    """Which blocks / fields differ (for the assertion message)."""
    _, _, bs, fields = TYPES[tag]
    a, b = out.reshape(-1, bs), want.reshape(-1, bs)
    bad = np.flatnonzero((a != b).any(axis=1))
    what = {k: int((a[bad][:, s] != b[bad][:, s]).sum()) for k, s in fields.items()}
    return f"{tag}: {bad.size} of {a.shape[0]} blocks differ (first {bad[:4].tolist()}, K={K}): bytes per field {what}"


def test_fixture_files_are_intact():
    assert len(MANIFEST["files"]) == 14
    for name, meta in MANIFEST["files"].items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"], name
        assert hashlib.sha256(blob.tobytes()).hexdigest() == meta["sha256"], name


def test_python_tables_know_the_types():
    assert (G.GGML_TYPE_Q2_K, G.GGML_TYPE_Q3_K) == (Q2_K, Q3_K)
    assert G.TYPE_BY_NAME["q2_K"] == Q2_K and G.TYPE_BY_NAME["q3_K"] == Q3_K
    assert G.BLOCK[Q2_K] == (256, 84) and G.BLOCK[Q3_K] == (256, 110)
    assert G.row_size(Q2_K, 11008) == 43 * 84 == 3612 and G.row_size(Q3_K, 11008) == 43 * 110 == 4730
    assert gpt2mod.FTYPES["q2_k"] == (10, Q2_K) and gpt2mod.FTYPES["q3_k"] == (11, Q3_K)


@pytest.mark.parametrize("tag", TAGS)
def test_type_traits(rt, tag):
    t, name, bs, _ = TYPES[tag]
    assert rt.ggml_type_name(t) == name
    assert rt.ggml_blck_size(t) == 256 and rt.ggml_type_size(t) == bs
    for K in (256, 768, 4096, 11008):
        assert rt.ggml_row_size(t, K) == K // 256 * bs


@needs_ref
@pytest.mark.parametrize("tag", TAGS)
def test_type_traits_match_reference(rt, ref, tag):
    t = TYPES[tag][0]
    assert rt.ggml_type_name(t) == ref.ggml_type_name(t)
    assert rt.ggml_blck_size(t) == ref.ggml_blck_size(t)
    assert rt.ggml_type_size(t) == ref.ggml_type_size(t)
    for K in (256, 2816, 11008):
        assert rt.ggml_row_size(t, K) == ref.ggml_row_size(t, K)


@pytest.mark.parametrize("which", ["w", "edge"])
@pytest.mark.parametrize("tag", TAGS)
def test_quantize_chunk_matches_golden_bytes(rt, tag, which):
    K = MANIFEST[which]["K"]
    out = quantize(rt, TYPES[tag][0], golden_blob(f"{tag}_{which}.f32", np.float32), K)
    if INSTRUMENTED:
        return
    want = golden_blob(f"{tag}_{which}.wq.bin")
    assert np.array_equal(out, want), describe(tag, out, want, K)


@pytest.mark.parametrize("tag", TAGS)
def test_quantize_chunk_start_offset(rt, tag):
    """Rows quantized in two calls (start = 0 and start = 3 rows) land where one call puts them."""
    t = TYPES[tag][0]
    K, N = MANIFEST["w"]["K"], MANIFEST["w"]["N"]
    w = golden_blob(f"{tag}_w.f32", np.float32)
    rs = G.row_size(t, K)
    out = np.zeros(rs * N, np.uint8)
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, 3, K, None) == 3 * rs
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 3 * K, N - 3, K, None) == (N - 3) * rs
    assert np.array_equal(out, quantize(rt, t, w, K))


@pytest.mark.parametrize("tag", TAGS)
def test_all_zero_input_is_all_zero_bytes(rt, tag):
    out = quantize(rt, TYPES[tag][0], np.zeros(512, np.float32), 512)
    assert not out.any()


def _edge_rows(K):
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    rows.append(np.abs(synth.uniform(40, K)) + 0.5)                                       # all positive: Q2_K mins 0
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)      # negative largest scale
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)     # positive largest scale
    r = synth.uniform(44, K).copy(); r[32:48] = 0.0; rows.append(r)                       # one zero sub-block
    r = synth.uniform(45, K).copy(); r[:256] = 0.0; rows.append(r)                        # zero superblock first
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # zero d
    r = (synth.uniform(48, K) * 3e-5).astype(np.float32); rows.append(r)                  # fp16-subnormal d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)
    return np.stack([np.asarray(r, np.float32) for r in rows])


@needs_ref
@pytest.mark.parametrize("K", [256, 768, 2816])
@pytest.mark.parametrize("tag", TAGS)
def test_quantize_chunk_matches_reference(rt, ref, tag, K):
    if INSTRUMENTED:
        pytest.skip("instrumented host build: bytes follow the release flags' FMA contraction")
    t = TYPES[tag][0]
    rng = np.random.default_rng(2000 + K)
    n = max(4, 16384 // K)
    w = np.concatenate([rng.standard_normal(n * K).astype(np.float32),
                        (rng.standard_normal(4 * K) * rng.uniform(1e-3, 30.0, 4 * K)).astype(np.float32),
                        _edge_rows(K).ravel()])
    out, want = quantize(rt, t, w, K), quantize(ref, t, w, K)
    assert np.array_equal(out, want), describe(tag, out, want, K)
