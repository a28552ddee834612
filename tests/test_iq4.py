"""CPU tests of the IQ4_NL / IQ4_XS host side (no GPU): ggml_quantize_chunk writes the reference's
bytes -- against the committed fixtures (tests/golden/iq4nl_*, iq4xs_*, written by
tests/golden/make_iq4_golden.py from the reference build) everywhere, and against the reference
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
IQ4_NL, IQ4_XS = 20, 23
# tag, ggml type, name, block elements, block bytes, the block's fields
TYPES = {
    "iq4nl": (IQ4_NL, b"iq4_nl", 32, 18, {"d": slice(0, 2), "qs": slice(2, 18)}),
    "iq4xs": (IQ4_XS, b"iq4_xs", 256, 136, {"d": slice(0, 2), "scales_h": slice(2, 4), "scales_l": slice(4, 8), "qs": slice(8, 136)}),
}
TAGS = list(TYPES)

with open(os.path.join(GOLDEN, "iq4.json")) as _f:
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
    bs, fields = TYPES[tag][3], TYPES[tag][4]
    a, b = out.reshape(-1, bs), want.reshape(-1, bs)
    bad = np.flatnonzero((a != b).any(axis=1))
    what = {k: int((a[bad][:, s] != b[bad][:, s]).sum()) for k, s in fields.items()}
    return f"{tag}: {bad.size} of {a.shape[0]} blocks differ (first {bad[:4].tolist()}, K={K}): bytes per field {what}"


def test_fixture_files_are_intact():
    assert len(MANIFEST["files"]) == 14
    for name, meta in MANIFEST["files"].items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"], name
        assert blob.nbytes <= 24 * 1024, name
        assert hashlib.sha256(blob.tobytes()).hexdigest() == meta["sha256"], name


def test_python_tables_know_the_types():
    assert (G.GGML_TYPE_IQ4_NL, G.GGML_TYPE_IQ4_XS) == (IQ4_NL, IQ4_XS)
    assert G.TYPE_BY_NAME["iq4_nl"] == IQ4_NL and G.TYPE_BY_NAME["iq4_xs"] == IQ4_XS
    assert G.BLOCK[IQ4_NL] == (32, 18) and G.BLOCK[IQ4_XS] == (256, 136)
    assert G.row_size(IQ4_NL, 11008) == 344 * 18 == 6192 and G.row_size(IQ4_XS, 11008) == 43 * 136 == 5848
    assert G.row_size(IQ4_XS, 11008) % 16 == 8
    assert gpt2mod.FTYPES["iq4_nl"] == (19, IQ4_NL) and gpt2mod.FTYPES["iq4_xs"] == (22, IQ4_XS)


@pytest.mark.parametrize("tag", TAGS)
def test_type_traits(rt, tag):
    t, name, blck, bs, _ = TYPES[tag]
    assert rt.ggml_type_name(t) == name
    assert rt.ggml_blck_size(t) == blck and rt.ggml_type_size(t) == bs
    assert rt.ggml_is_quantized(t)
    assert not rt.ggml_quantize_requires_imatrix(t)
    for K in (256, 768, 4096, 11008):
        assert rt.ggml_row_size(t, K) == K // blck * bs


@needs_ref
@pytest.mark.parametrize("tag", TAGS)
def test_type_traits_match_reference(rt, ref, tag):
    t = TYPES[tag][0]
    assert rt.ggml_type_name(t) == ref.ggml_type_name(t)
    assert rt.ggml_blck_size(t) == ref.ggml_blck_size(t)
    assert rt.ggml_type_size(t) == ref.ggml_type_size(t)
    assert bool(rt.ggml_quantize_requires_imatrix(t)) == bool(ref.ggml_quantize_requires_imatrix(t))
    for K in (256, 2816, 11008):
        assert rt.ggml_row_size(t, K) == ref.ggml_row_size(t, K)


@pytest.mark.parametrize("ftype,t", [(19, IQ4_NL), (22, IQ4_XS)])
def test_ftype_to_type(rt, ftype, t):
    assert rt.ggml_ftype_to_ggml_type(ftype) == t


@needs_ref
@pytest.mark.parametrize("ftype", [19, 22])
def test_ftype_to_type_matches_reference(rt, ref, ftype):
    assert rt.ggml_ftype_to_ggml_type(ftype) == ref.ggml_ftype_to_ggml_type(ftype)


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


def test_all_zero_input_bytes(rt):
    """Zero input is not zero bytes: index 8 (the level 1) is the nearest to 0, and IQ4_XS's
    d = -max_scale / 32 is fp16 -0.0 with every 6-bit scale 32 (scales_h 0xAAAA, scales_l 0)."""
    nl = quantize(rt, IQ4_NL, np.zeros(64, np.float32), 64).reshape(2, 18)
    assert (nl[:, 0:2] == 0).all() and (nl[:, 2:] == 0x88).all()
    xs = quantize(rt, IQ4_XS, np.zeros(512, np.float32), 512).reshape(2, 136)
    assert (xs[:, 0] == 0x00).all() and (xs[:, 1] == 0x80).all()
    assert (xs[:, 2:4] == 0xAA).all() and (xs[:, 4:8] == 0).all() and (xs[:, 8:] == 0x88).all()


@pytest.mark.parametrize("tag", TAGS)
def test_codebook_row_uses_all_sixteen_codes(tag):
    """The last edge row (kvalues and its reverse times 0.01, tiled): every code in both nibble halves."""
    K, N = MANIFEST["edge"]["K"], MANIFEST["edge"]["N"]
    bs = TYPES[tag][3]
    row = golden_blob(f"{tag}_edge.wq.bin").reshape(N, -1)[N - 1].reshape(-1, bs)
    qs = row[:, TYPES[tag][4]["qs"]]
    assert set((qs & 15).ravel().tolist()) == set(range(16)) and set((qs >> 4).ravel().tolist()) == set(range(16))


def _edge_rows(K):
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    rows.append(np.abs(synth.uniform(40, K)) + 0.5)                                       # all positive
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)
    r = synth.uniform(44, K).copy(); r[32:64] = 0.0; rows.append(r)                       # one zero block
    r = synth.uniform(45, K).copy(); r[:256] = 0.0; rows.append(r)                        # zero superblock first
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # zero d
    r = (synth.uniform(48, K) * 3e-3).astype(np.float32); rows.append(r)                  # fp16-subnormal d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)
    return np.stack([np.asarray(r, np.float32) for r in rows])


@needs_ref
@pytest.mark.parametrize("K", [256, 768, 4096, 11008])
@pytest.mark.parametrize("tag", TAGS)
def test_quantize_chunk_matches_reference(rt, ref, tag, K):
    if INSTRUMENTED:
        pytest.skip("instrumented host build: bytes follow the release flags' FMA contraction")
    t = TYPES[tag][0]
    rng = np.random.default_rng(2000 + K)
    n = max(4, 16384 // K)
    w = np.concatenate([rng.standard_normal(n * K).astype(np.float32),
                        (rng.standard_normal(4 * K) * rng.uniform(1e-3, 30.0, 4 * K)).astype(np.float32),
                        (rng.standard_normal(2 * K) * np.repeat(10.0 ** rng.uniform(-8, 4, 2 * K // 32), 32)).astype(np.float32),
                        _edge_rows(K).ravel()])
    out, want = quantize(rt, t, w, K), quantize(ref, t, w, K)
    assert np.array_equal(out, want), describe(tag, out, want, K)
