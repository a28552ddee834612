"""The quantized weight types under test, one table row each, and what their tests share: fixtures,
comparison helpers, graph builders and, as check_* functions over a table row, the bodies of the
tests that several families have. The test files (tests/test_q6k*.py, test_legacy_quants*.py,
test_q2k_q3k*.py, test_iq4*.py) parametrize over their family's rows and call the checks; a value
that differs between types (shapes, column counts, batch sizes) is a field of the row.

To add a type: add a row to TYPES (a new family also a dict of the fields its types share), commit
its fixtures under tests/golden/ (the quantized rows, their dequantization and the reference output
of the "w" and "edge" cases, listed in the family's manifest), a builder of hand-made blocks for
`block` if the family is new, and in the family's two test files the tests that call the checks.
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
from dataclasses import dataclass
from typing import Callable, Optional

os.environ.setdefault("GGML_MI355X_SPLIT_SLOTS", "3")  # read once, at the first split buffer type (as tests/test_split_gpu.py)

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_blob
from ggml_mi355x import ggml as G
from ggml_mi355x import gguf
from ggml_mi355x import gpt2
from ggml_mi355x import gpt2 as gpt2mod
from ggml_mi355x import synth

REF = os.path.join(REPO, "oracle", "_ref")
REF_LIB = os.path.join(REF, "libggml_ref.so")
REF_GPT2 = os.path.join(REF, "libgpt2_ref.so")
REF_QUANTIZE = os.path.join(REF, "gpt-2-quantize")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference lib not built (make -C oracle ref)")
# an instrumented build of the host runtime: the bytes of the quantizers marked fma_sensitive follow
# gcc's FMA contraction of the release flags, which instrumentation can change (as tests/test_core.py)
INSTRUMENTED = bool(os.environ.get("GGML_MI355X_CORE_LIB"))
TREE_TOL = 1e-5  # integer block sums are exact: only the f32 combination order differs
Q8_0, Q8_1, Q8_K = 8, 9, 15


# ------------------------------------------------------------------ hand-made blocks

def _f16(v):
    return np.array([v], np.float16).view(np.uint8)


def _filled(n, nbytes, d_at, fill, d=1.0):
    """n blocks (256 elements) whose bytes are all `fill` (0x00 or 0xFF) but for the fp16 d at each of d_at.
    Q2_K: every scale and min 0 / 15 and every q 0 / 3; Q3_K: every sc - 32 = -32 / 31 and every
    q - 4 * !hbit = -4 / 3; IQ4: every code 0 (the level -127) / 15 (113) and, IQ4_XS, every ls = 0
    (the scale -32) / 63 (31)."""
    b = np.full((n, nbytes), fill, np.uint8)
    for at in d_at:
        b[:, at:at + 2] = _f16(d)
    return b.ravel()


def _q6k_block(fill, d=1.0):
    """ql and qh all `fill`: every q - 32 = -32 under scales of -128 (0x00), 31 under scales of 127 (0xFF)."""
    b = _filled(1, 210, (208,), fill, d)
    b[192:208] = np.array([127 if fill else -128], np.int8).view(np.uint8)[0]
    return b


def _legacy_block(t, qs, qh=0, d=1.0, m=0.5):
    """One hand-made block: qs 16 bytes (or one value for all), qh the 32 fifth bits."""
    parts = [_f16(d)]
    if t != 6:
        parts.append(_f16(m))
    if t != 3:
        parts.append(np.array([qh], "<u4").view(np.uint8))
    parts.append(np.broadcast_to(np.asarray(qs, np.uint8), (16,)))
    b = np.concatenate(parts)
    assert b.size == G.BLOCK[t][1]
    return b


# ------------------------------------------------------------------ the table

@dataclass(frozen=True, eq=False)
class WeightType:
    tag: str                # the test ids' prefix
    type: int               # ggml type id
    name: str               # ggml's type name
    family: str             # the golden manifest tests/golden/<family>.json
    ftype: int              # the model file's ftype; the quantize_model name is the lower-case type name
    act: int                # the vec_dot type: what MUL_MAT quantizes src1 to
    blck: int               # elements per block
    block_bytes: int        # bytes per block
    fields: dict            # the block's fields, for the messages of the quantizer tests
    block: Callable         # the family's hand-made block builder
    blob: str               # prefix of the fixtures of the quantized rows; `f32` that of their f32 inputs
    f32: str
    fma_sensitive: bool     # see INSTRUMENTED
    # CPU tests
    trait_K: tuple
    ref_trait_K: tuple
    quant_K: tuple
    # GPU tests
    shapes: tuple           # (K, N) of the two MUL_MAT sweeps, each over `cols` columns
    cols: tuple
    ffn_down_N: int
    batch_K: int            # K of the 3-D weight batch
    prequant_B: tuple
    chain_B: tuple
    gpt2_modes: tuple       # "decode" (over gpt2_decode tokens), "prompt<n>" in one batch, "batches_of_8"
    gpt2_decode: int
    split_B: tuple
    id_tokens: Optional[tuple] = None  # n_tokens of the MUL_MAT_ID test, where the type has one
    cpy_strict: bool = False           # the CPY -> MUL_MAT graph is also held against the F32-src1 path and the extreme blocks
    gguf_get_rows: bool = False        # the GGUF test reads the tensor through GET_ROWS as well

    @property
    def model(self):
        return self.name.lower()

    @property
    def manifest(self):
        return MANIFESTS[self.family]

    def golden(self, suffix, dtype=np.uint8):
        return golden_blob(f"{self.blob}_{suffix}", dtype)

    def source(self, which):
        return golden_blob(f"{self.f32}_{which}.f32", np.float32)


MANIFESTS = {}
for _family in ("q6k", "legacy", "q2k_q3k", "iq4"):
    with open(os.path.join(GOLDEN, _family + ".json")) as _f:
        MANIFESTS[_family] = json.load(_f)

# Superblock types: rows of 2 mod 4 (Q6_K, Q3_K) or 4-byte-only (Q2_K) alignment with the odd superblock
# counts 1, 3, 11; under one / exactly one / one and a half items per lane of a wave (K 2048 / 4096 /
# 6144); N not a multiple of 4 or of the rows per workgroup; 1..8 columns in one launch, the 4-column
# split, 8-column chunks with a ragged tail.
_K_QUANT = dict(
    blck=256, act=Q8_K, fma_sensitive=True, trait_K=(256, 768, 4096, 11008), ref_trait_K=(256, 2816, 11008), quant_K=(256, 768, 2816),
    shapes=((256, 5), (768, 67), (2048, 67), (2816, 33), (4096, 67), (6144, 9)), cols=(1, 2, 3, 5, 8, 9, 17), ffn_down_N=10,
    prequant_B=(4, 20), chain_B=(1, 3), gpt2_modes=("decode", "prompt20", "batches_of_8"), gpt2_decode=12, split_B=(1, 12))
_Q2K_Q3K = dict(_K_QUANT, family="q2k_q3k", batch_K=768, id_tokens=(1, 12), cpy_strict=True)  # K 768: Q3_K rows 2 mod 4
# 32-element blocks: one block; ragged K (3 blocks); an odd block count whose Q5_0 rows are 2 mod 4 (25
# blocks = 550 B); under one, exactly one and one and a half blocks per lane pair of a wave; the columns as above.
_LEGACY = dict(
    _K_QUANT, family="legacy", f32="legacy", blck=32, fma_sensitive=False, batch_K=512, gguf_get_rows=True,
    trait_K=(32, 96, 4096, 11008), ref_trait_K=(32, 800, 11008), quant_K=(32, 96, 4096),
    shapes=((32, 5), (96, 67), (800, 33), (2048, 67), (4096, 67), (6144, 9)))
# IQ4: one superblock; one item per lane of a wave (K 4096: IQ4_NL two); 43 superblocks, 5848-byte IQ4_XS
# rows (8 mod 16) and more than two items per lane (K 11008); N not a multiple of the rows per
# workgroup. IQ4_NL also rows that are no multiple of 256 (an even block count: 2 and 10 blocks), which
# only the generic kernels take. 1..8 columns in one launch, 8-column chunks with a tail of 1, and two
# whole chunks.
_IQ4_SHAPES = ((256, 33), (4096, 64), (11008, 16))
_IQ4 = dict(
    family="iq4", fma_sensitive=True, trait_K=(256, 768, 4096, 11008), ref_trait_K=(256, 2816, 11008), quant_K=(256, 768, 4096, 11008),
    cols=(1, 2, 5, 8, 9, 16), ffn_down_N=64, batch_K=768, prequant_B=(1, 4), chain_B=(1, 8), id_tokens=(1, 5),
    gpt2_modes=("decode", "prompt12"), gpt2_decode=8, split_B=(1, 16), cpy_strict=True)  # K 768: IQ4_XS rows 8 mod 16


def _legacy(name, t, ftype, act, nbytes, fields):
    return WeightType(name, t, name, ftype=ftype, block_bytes=nbytes, fields=fields, blob="legacy_" + name,
                      block=functools.partial(_legacy_block, t), **dict(_LEGACY, act=act))


TYPES = [
    WeightType("q6k", 14, "q6_K", ftype=14, block_bytes=210, blob="q6k", f32="q6k", block=_q6k_block,
               fields={"ql": slice(0, 128), "qh": slice(128, 192), "scales": slice(192, 208), "d": slice(208, 210)},
               **dict(_K_QUANT, family="q6k", batch_K=512)),
    _legacy("q4_1", 3, 3, Q8_1, 20, {"d": slice(0, 2), "m": slice(2, 4), "qs": slice(4, 20)}),
    _legacy("q5_0", 6, 8, Q8_0, 22, {"d": slice(0, 2), "qh": slice(2, 6), "qs": slice(6, 22)}),
    _legacy("q5_1", 7, 9, Q8_1, 24, {"d": slice(0, 2), "m": slice(2, 4), "qh": slice(4, 8), "qs": slice(8, 24)}),
    WeightType("q2k", 10, "q2_K", ftype=10, block_bytes=84, blob="q2k", f32="q2k", block=functools.partial(_filled, 1, 84, (80, 82)),
               fields={"scales": slice(0, 16), "qs": slice(16, 80), "d": slice(80, 82), "dmin": slice(82, 84)}, **_Q2K_Q3K),
    WeightType("q3k", 11, "q3_K", ftype=11, block_bytes=110, blob="q3k", f32="q3k", block=functools.partial(_filled, 1, 110, (108,)),
               fields={"hmask": slice(0, 32), "qs": slice(32, 96), "scales": slice(96, 108), "d": slice(108, 110)}, **_Q2K_Q3K),
    WeightType("iq4nl", 20, "iq4_nl", ftype=19, act=Q8_0, blck=32, block_bytes=18, blob="iq4nl", f32="iq4nl",
               block=functools.partial(_filled, 8, 18, (0,)), fields={"d": slice(0, 2), "qs": slice(2, 18)},
               shapes=_IQ4_SHAPES + ((64, 16), (320, 40)), **_IQ4),
    WeightType("iq4xs", 23, "iq4_xs", ftype=22, act=Q8_K, blck=256, block_bytes=136, blob="iq4xs", f32="iq4xs",
               block=functools.partial(_filled, 1, 136, (0,)), shapes=_IQ4_SHAPES,
               fields={"d": slice(0, 2), "scales_h": slice(2, 4), "scales_l": slice(4, 8), "qs": slice(8, 136)}, **_IQ4),
]


def rows(*names):
    """The rows of the named tags or families, in table order; all of them without a name."""
    return [wt for wt in TYPES if not names or wt.tag in names or wt.family in names]


# ------------------------------------------------------------------ fixtures

@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def backend(rt):
    b = G.mi355x_backend(rt, 0)
    yield b
    rt.ggml_backend_free(b)


@pytest.fixture(scope="module")
def ref():
    """The reference library, loaded isolated beside the runtime, and its CPU backend."""
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


# ------------------------------------------------------------------ helpers

def rel_err(y, r):
    return float(np.abs(y.astype(np.float64) - r).max() / max(np.abs(r).max(), 1e-30))


def same_bits(y, r):
    return np.array_equal(y.view(np.uint32), r.view(np.uint32))


def in_order(rt, order, fn):
    assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
    try:
        return fn()
    finally:
        rt.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)


def quantize(lib, t, w, K):
    w = np.ascontiguousarray(w, np.float32)
    n = w.size // K
    out = np.empty(G.row_size(t, K) * n, np.uint8)
    assert lib.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, n, K, None) == out.nbytes
    return out


@functools.lru_cache(maxsize=None)
def weights(T, K, N, seed):
    """Seeded rows of type T from the runtime's quantizer (the CPU tests of each type pin it to the reference's bytes)."""
    out = quantize(G.runtime(), T, np.random.default_rng(seed).standard_normal(K * N).astype(np.float32), K)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_mul_mat(T, K, N, B):
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    try:
        y = G.mul_mat_once(lib, cpu, T, weights(T, K, N, 100 + K + N), K, N, synth.uniform(200 + K + B, K * B), B)
    finally:
        lib.ggml_backend_free(cpu)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------ graph builders

def _compute(lib, backend, c, outs, inputs):
    """Allocate the context's tensors on the backend, set the inputs, run the graph of outs, read them back."""
    g = lib.ggml_new_graph(c.ctx)
    for y in outs:
        lib.ggml_build_forward_expand(g, y)
    buf = lib.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
    assert buf
    try:
        for t, a in inputs:
            G.tensor_set(lib, t, a)
        assert lib.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
        return [G.tensor_get(lib, y) for y in outs]
    finally:
        lib.ggml_backend_buffer_free(buf)


def _mul_mat_general(lib, backend, T, wq, w_ne, x, x_ne, permute_x):
    """W [K, N, ne02, 1] x X [K, ne11, ne12, 1] with broadcasting; permute_x: X stored as
    [K, ne12, ne11] and permuted, so that src1's columns are strided."""
    ovh = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, ovh, no_alloc=True) as c:
        w = lib.ggml_new_tensor_4d(c.ctx, T, *w_ne)
        if permute_x:
            xs = lib.ggml_new_tensor_4d(c.ctx, G.GGML_TYPE_F32, x_ne[0], x_ne[2], x_ne[1], x_ne[3])
            xt = lib.ggml_permute(c.ctx, xs, 0, 2, 1, 3)
        else:
            xs = xt = lib.ggml_new_tensor_4d(c.ctx, G.GGML_TYPE_F32, *x_ne)
        return _compute(lib, backend, c, [lib.ggml_mul_mat(c.ctx, w, xt)], [(w, wq), (xs, x)])[0]


def _cpy_then_mul_mat(lib, backend, wt, wq, K, N, x, B):
    """X (f32) -> CPY to rows of the weight's vec_dot type -> MUL_MAT(W, Xq) as one graph."""
    overhead = lib.ggml_tensor_overhead() * 8 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        w = lib.ggml_new_tensor_2d(c.ctx, wt.type, K, N)
        xt = lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, B)
        xq = lib.ggml_cpy(c.ctx, xt, lib.ggml_new_tensor_2d(c.ctx, wt.act, K, B))
        return _compute(lib, backend, c, [lib.ggml_mul_mat(c.ctx, w, xq)], [(w, wq), (xt, x)])[0]


def _three_mul_mats(lib, backend, T, wqs, K, N, xs):
    """Three independent same-shape mul_mats (B = 1) in one graph."""
    overhead = lib.ggml_tensor_overhead() * 16 + lib.ggml_graph_overhead()
    with G.Context(lib, overhead, no_alloc=True) as c:
        ws = [lib.ggml_new_tensor_2d(c.ctx, T, K, N) for _ in wqs]
        xts = [lib.ggml_new_tensor_2d(c.ctx, G.GGML_TYPE_F32, K, 1) for _ in xs]
        ys = [lib.ggml_mul_mat(c.ctx, w, x) for w, x in zip(ws, xts)]
        return _compute(lib, backend, c, ys, list(zip(ws, wqs)) + list(zip(xts, xs)))


def _mul_mat_id(L, be, T, w, K, n, n_as, n_ids, n_tokens, x, ids):
    def build(c):
        a = L.ggml_new_tensor_3d(c, T, K, n, n_as)
        b = L.ggml_new_tensor_3d(c, G.GGML_TYPE_F32, K, 1, n_tokens)
        full = L.ggml_new_tensor_2d(c, G.GGML_TYPE_I32, n_as, n_tokens)
        top = L.ggml_view_2d(c, full, n_ids, n_tokens, full.contents.nb[1], 0)
        return [(a, w), (b, x), (full, ids)], L.ggml_mul_mat_id(c, a, b, top)
    return G.graph_once(L, be, build)


def _both_models(path, n_batch):
    lib = G.runtime()
    be = G.mi355x_backend(lib)
    ours = gpt2.Model(lib, path, be, n_batch=n_batch)
    ref = G.Lib([REF_LIB, REF_GPT2], isolated=True)
    rbe = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(rbe, 4)
    rm = gpt2.Model(ref, path, rbe, n_batch=n_batch)

    def free():
        ours.free()
        rm.free()
        lib.ggml_backend_free(be)
        ref.ggml_backend_free(rbe)
    return ours, rm, free


def _split_buft(rt, props):
    arr = (ctypes.c_float * 16)(*([float(p) for p in props] + [0.0] * (16 - len(props))))
    return rt.ggml_backend_mi355x_split_buffer_type(ctypes.cast(arr, ctypes.c_void_p))


# ------------------------------------------------------------------ the shared CPU test bodies (ref: the reference library alone)

def ftype_to_type(lib, ftype):
    for h in lib.handles:
        if hasattr(h, "ggml_ftype_to_ggml_type"):
            return int(h.ggml_ftype_to_ggml_type(ftype))
    raise AssertionError("ggml_ftype_to_ggml_type is not exported")


def describe(wt, out, want, K):
    """Which blocks / fields differ (for the assertion message)."""
    a, b = out.reshape(-1, wt.block_bytes), want.reshape(-1, wt.block_bytes)
    bad = np.flatnonzero((a != b).any(axis=1))
    what = {k: int((a[bad][:, s] != b[bad][:, s]).sum()) for k, s in wt.fields.items()}
    return f"{wt.tag}: {bad.size} of {a.shape[0]} blocks differ (first {bad[:4].tolist()}, K={K}): bytes per field {what}"


def check_fixture_files_are_intact(family):
    files = MANIFESTS[family]["files"]
    n_files, max_bytes = {"q2k_q3k": (14, None), "iq4": (14, 24 * 1024)}.get(family, (None, None))
    assert n_files is None or len(files) == n_files
    for name, meta in files.items():
        blob = golden_blob(name)
        assert blob.nbytes == meta["bytes"], name
        assert max_bytes is None or blob.nbytes <= max_bytes, name
        assert hashlib.sha256(blob.tobytes()).hexdigest() == meta["sha256"], name


def check_python_tables_know_the_types(family):
    for wt in rows(family):
        t = wt.type
        assert getattr(G, "GGML_TYPE_" + wt.name.upper()) == t and G.TYPE_BY_NAME[wt.name] == t
        assert G.BLOCK[t] == (wt.blck, wt.block_bytes)
        assert G.row_size(t, 11008) == 11008 // wt.blck * wt.block_bytes
        assert gpt2mod.FTYPES[wt.model] == (wt.ftype, t)
    if family == "legacy":
        assert G.GGML_TYPE_Q8_1 == Q8_1 and G.BLOCK[Q8_1] == (32, 36)
    if family == "iq4":
        assert G.row_size(23, 11008) == 5848 and G.row_size(23, 11008) % 16 == 8


def check_type_traits(rt, wt):
    t = wt.type
    assert rt.ggml_type_name(t) == wt.name.encode()
    assert rt.ggml_blck_size(t) == wt.blck and rt.ggml_type_size(t) == wt.block_bytes
    for K in wt.trait_K:
        assert rt.ggml_row_size(t, K) == K // wt.blck * wt.block_bytes
    if wt.family == "iq4":
        assert rt.ggml_is_quantized(t)
        assert not rt.ggml_quantize_requires_imatrix(t)
    if wt.family == "legacy":
        assert ftype_to_type(rt, wt.ftype) == t
        assert rt.ggml_type_size(Q8_1) == 36 and rt.ggml_blck_size(Q8_1) == 32


def check_type_traits_match_reference(rt, ref, wt):
    t = wt.type
    assert rt.ggml_type_name(t) == ref.ggml_type_name(t)
    assert rt.ggml_blck_size(t) == ref.ggml_blck_size(t)
    assert rt.ggml_type_size(t) == ref.ggml_type_size(t)
    for K in wt.ref_trait_K:
        assert rt.ggml_row_size(t, K) == ref.ggml_row_size(t, K)
    if wt.family == "iq4":
        assert bool(rt.ggml_quantize_requires_imatrix(t)) == bool(ref.ggml_quantize_requires_imatrix(t))
    if wt.family == "legacy":
        assert ftype_to_type(rt, wt.ftype) == ftype_to_type(ref, wt.ftype)


def check_quantize_chunk_matches_golden_bytes(rt, wt, which):
    K = wt.manifest[which]["K"]
    out = quantize(rt, wt.type, wt.source(which), K)
    if INSTRUMENTED and wt.fma_sensitive:
        return
    want = wt.golden(f"{which}.wq.bin")
    assert np.array_equal(out, want), describe(wt, out, want, K)


def check_quantize_chunk_start_offset(rt, wt):
    """Rows quantized in two calls (start = 0 and start = 3 rows) land where one call puts them."""
    t, K, N = wt.type, wt.manifest["w"]["K"], wt.manifest["w"]["N"]
    w = wt.source("w")
    rs = G.row_size(t, K)
    out = np.zeros(rs * N, np.uint8)
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 0, 3, K, None) == 3 * rs
    assert rt.ggml_quantize_chunk(t, w.ctypes.data, out.ctypes.data, 3 * K, N - 3, K, None) == (N - 3) * rs
    assert np.array_equal(out, quantize(rt, t, w, K))


def check_all_zero_input_is_all_zero_bytes(rt, wt):
    out = quantize(rt, wt.type, np.zeros(512, np.float32), 512)
    assert not out.any()


def _edge_rows(K, zero_run=slice(32, 48), subnormal=None):
    """The superblock families' edge rows. Q6_K has neither the all-positive row nor the fp16-subnormal one."""
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    if subnormal:
        rows.append(np.abs(synth.uniform(40, K)) + 0.5)                                   # all positive: Q2_K mins 0
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)      # negative largest scale
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)     # positive largest scale
    r = synth.uniform(44, K).copy(); r[zero_run] = 0.0; rows.append(r)                    # one zero sub-block / block
    r = synth.uniform(45, K).copy(); r[:256] = 0.0; rows.append(r)                        # zero superblock first
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # zero d
    if subnormal:
        r = (synth.uniform(48, K) * subnormal).astype(np.float32); rows.append(r)         # fp16-subnormal d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)
    return np.stack([np.asarray(r, np.float32) for r in rows])


def _legacy_edge_rows(K):
    rows = [np.zeros(K, np.float32), np.full(K, -1.25, np.float32)]
    r = (synth.uniform(41, K) * 1e-3).astype(np.float32); r[K // 2 + 3] = 1e4; rows.append(r)
    r = (synth.uniform(42, K) * 0.1).astype(np.float32); r[17] = 5.0; rows.append(r)
    r = (synth.uniform(43, K) * 0.1).astype(np.float32); r[17] = -5.0; rows.append(r)
    r = synth.uniform(44, K).copy(); r[3] = -2.0; r[9] = 2.0; rows.append(r)              # +a and -a both largest
    r = (synth.uniform(46, K) * 1e-20).astype(np.float32); rows.append(r)                 # fp16-subnormal / zero d
    r = (synth.uniform(47, K) * 6e4).astype(np.float32); rows.append(r)                   # d near the fp16 range
    r = np.abs(synth.uniform(48, K)) + 3.0; rows.append(r.astype(np.float32))             # large positive min
    return np.stack(rows)


def _quantizer_input(wt, K):
    """Random rows (plain and widely scaled; IQ4: also scaled block by block over twelve decades) and
    the family's edge rows; the 32-element types some thousand blocks of each."""
    if wt.family == "legacy":
        rng, n, edge = np.random.default_rng(1000 + K + wt.type), max(4, 65536 // K), _legacy_edge_rows(K)
        scaled = n
    else:
        rng = np.random.default_rng(1000 + K if wt.family == "q6k" else 2000 + K)
        n, scaled = max(4, 16384 // K), 4
        edge = {"q6k": lambda: _edge_rows(K), "q2k_q3k": lambda: _edge_rows(K, subnormal=3e-5),
                "iq4": lambda: _edge_rows(K, slice(32, 64), 3e-3)}[wt.family]()
    parts = [rng.standard_normal(n * K).astype(np.float32),
             (rng.standard_normal(scaled * K) * rng.uniform(1e-3, 30.0, scaled * K)).astype(np.float32)]
    if wt.family == "iq4":
        parts.append((rng.standard_normal(2 * K) * np.repeat(10.0 ** rng.uniform(-8, 4, 2 * K // 32), 32)).astype(np.float32))
    return np.concatenate(parts + [edge.ravel()])


def check_quantize_chunk_matches_reference(rt, ref, wt, K):
    if INSTRUMENTED and wt.fma_sensitive:
        pytest.skip("instrumented host build: bytes follow the release flags' FMA contraction")
    w = _quantizer_input(wt, K)
    out, want = quantize(rt, wt.type, w, K), quantize(ref, wt.type, w, K)
    if wt.family == "legacy":
        assert out.size // wt.block_bytes >= 4096
    assert np.array_equal(out, want), describe(wt, out, want, K)


# ------------------------------------------------------------------ the shared GPU test bodies

# columns whose quantized activations are all of the largest magnitude: constant columns (every
# quant 127 or -127 in Q8_0; -128 in Q8_K, one more than the +-127 of a mixed-sign column),
# alternating signs (+-127), and a small constant
EXTREME_X = (lambda K: np.concatenate([np.full(K, 0.5, np.float32), np.full(K, -2.0, np.float32)]),
             lambda K: np.concatenate([np.tile(np.array([3.0, -3.0], np.float32), K // 2), np.full(K, 1e-3, np.float32)]))


TINY = dict(n_embd=256, n_head=4, n_layer=2, n_vocab=512, n_ctx=64)
TOKENS = [(37 * i * i + 11 * i + 5) % 511 for i in range(20)]


@pytest.fixture(scope="module")
def tiny_models(tmp_path_factory):
    """The synthetic f16 model file, and a function from a table row to its quantized file (made on first use)."""
    d = tmp_path_factory.mktemp("weight_types_gpt2")
    f16 = gpt2.write_synthetic_model(str(d / "tiny-f16.bin"), **TINY)
    made = {}

    def quantized(wt):
        if wt.tag not in made:
            made[wt.tag] = gpt2.quantize_model(G.runtime(), f16, str(d / f"tiny-{wt.model}.bin"), wt.model)
        return made[wt.tag]
    return f16, quantized


def check_get_rows_matches_golden_dequantization(rt, backend, wt, which):
    """Row indices out of order and repeated, f32 dst: dequantize_row_*'s bits, the -0.0 elements of
    IQ4_XS's all-zero superblock (edge row 0) included."""
    T, K, N = wt.type, wt.manifest[which]["K"], wt.manifest[which]["N"]
    wq = wt.golden(f"{which}.wq.bin")
    want = wt.golden(f"{which}.wdq.f32", np.float32).reshape(N, K)
    idx = np.array([N - 1, 0, 2, 2, 1, N - 1, 3, 0, N - 2], np.int32)
    if which == "edge" and wt.tag == "iq4xs":
        assert (want[0, :256].view(np.uint32) == 0x80000000).all()  # the fixture does hold the -0.0 superblock

    def build(c):
        w = rt.ggml_new_tensor_2d(c, T, K, N)
        i = rt.ggml_new_tensor_1d(c, G.GGML_TYPE_I32, len(idx))
        return [(w, wq), (i, idx)], rt.ggml_get_rows(c, w, i)

    y = G.graph_once(rt, backend, build).reshape(len(idx), K)
    assert same_bits(y, want[idx]), float(np.abs(y - want[idx]).max())


def check_mul_mat_matches_golden_output(rt, backend, wt):
    """The committed reference-CPU output (B = 3): identical bits in order 1, 1e-5 in tree order."""
    T, c = wt.type, wt.manifest["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wq = wt.golden("w.wq.bin")
    x = synth.uniform(c["xseed"], K * B)
    want = wt.golden("w.y.f32", np.float32)
    y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
    print(f"golden {wt.tag} B={B}: order 1 rel err {rel_err(y1, want):.2e}, tree order {rel_err(y0, want):.2e}")
    assert same_bits(y1, want), rel_err(y1, want)
    assert rel_err(y0, want) <= TREE_TOL


def check_mul_mat_reference_order_bit_identical(rt, backend, wt, shape):
    T, (K, N) = wt.type, shape
    wq = weights(T, K, N, 100 + K + N)
    for B in wt.cols:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        yr = _ref_mul_mat(T, K, N, B)
        assert same_bits(y, yr), (B, float(np.mean(y.view(np.uint32) == yr.view(np.uint32))), rel_err(y, yr))


def check_mul_mat_tree_order(rt, backend, wt, shape):
    T, (K, N) = wt.type, shape
    wq = weights(T, K, N, 100 + K + N)
    for B in wt.cols:
        x = synth.uniform(200 + K + B, K * B)
        y = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        err = rel_err(y, _ref_mul_mat(T, K, N, B))
        print(f"tree order {wt.tag} K={K} N={N} B={B}: rel err {err:.2e}")
        assert err <= TREE_TOL, (B, err)


def check_mul_mat_llama_ffn_down_rows(rt, backend, ref, wt):
    """K = 11008 (LLaMA-7B's ffn_down): 43 superblocks or 344 blocks a row, more than two items per lane.
    Q6_K's 9030-byte and Q3_K's 4730-byte rows start 2 mod 4 every other row, Q2_K's 3612-byte rows
    4 mod 16, IQ4_XS's 5848-byte rows 8 mod 16; the 32-element types' rows, no multiple of 256, go to
    the generic kernels. Decode and prompt column counts."""
    lib, cpu = ref
    T, K, N = wt.type, 11008, wt.ffn_down_N
    wq = weights(T, K, N, 801)
    for B in (1, 3, 8, 9):
        x = synth.uniform(802 + B, K * B)
        yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x, B)
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yr), (B, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (B, rel_err(y0, yr))


def check_weight_batch_and_strided_src1(rt, backend, ref, wt, ne11):
    """A 3-D weight batch (ne02 = 2) broadcast over ne12 = 4, contiguous and strided src1."""
    lib, cpu = ref
    T, K, N, ne02, ne12 = wt.type, wt.batch_K, 40, 2, 4
    w_ne, x_ne = (K, N, ne02, 1), (K, ne11, ne12, 1)
    wq = weights(T, K, N * ne02, 301)
    x = synth.uniform(302 + ne11, K * ne11 * ne12)
    for permute in (False, True):
        yr = _mul_mat_general(lib, cpu, T, wq, w_ne, x, x_ne, permute)
        y1 = in_order(rt, 1, lambda: _mul_mat_general(rt, backend, T, wq, w_ne, x, x_ne, permute))
        y0 = in_order(rt, 0, lambda: _mul_mat_general(rt, backend, T, wq, w_ne, x, x_ne, permute))
        assert same_bits(y1, yr), (permute, rel_err(y1, yr))
        assert rel_err(y0, yr) <= TREE_TOL, (permute, rel_err(y0, yr))


def check_prequantized_src1(rt, backend, ref, wt, B):
    """src1 already rows of the vec_dot type (Q8_0, Q8_1 or Q8_K), read as it lies."""
    lib, cpu = ref
    T, K, N = wt.type, 1024, 48
    wq = weights(T, K, N, 401)
    x = synth.uniform(402 + B, K * B)
    yr = _cpy_then_mul_mat(lib, cpu, wt, wq, K, N, x, B)
    y1 = in_order(rt, 1, lambda: _cpy_then_mul_mat(rt, backend, wt, wq, K, N, x, B))
    y0 = in_order(rt, 0, lambda: _cpy_then_mul_mat(rt, backend, wt, wq, K, N, x, B))
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
    if wt.cpy_strict:
        yf = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yf), rel_err(y1, yf)  # the same quants either way: the F32-src1 path's bits


def check_three_independent_mul_mats_in_one_graph(rt, backend, ref, wt):
    lib, cpu = ref
    T, K, N = wt.type, 4096, 64
    wqs = [weights(T, K, N, 500 + i) for i in range(3)]
    xs = [synth.uniform(510 + i, K) for i in range(3)]
    yr = _three_mul_mats(lib, cpu, T, wqs, K, N, xs)
    y1 = in_order(rt, 1, lambda: _three_mul_mats(rt, backend, T, wqs, K, N, xs))
    y0 = in_order(rt, 0, lambda: _three_mul_mats(rt, backend, T, wqs, K, N, xs))
    for i in range(3):
        assert same_bits(y1[i], yr[i]), (i, rel_err(y1[i], yr[i]))
        assert rel_err(y0[i], yr[i]) <= TREE_TOL, (i, rel_err(y0[i], yr[i]))


def check_extreme_integers(rt, backend, ref, wt):
    """Hand-made blocks at the ends of the integer range against the columns above (through an F32
    src1 and, but for Q6_K, through src1 pre-quantized by CPY alike). Identical bits in the reference
    order pin the int32 accumulation: Q6_K with every q - 32 = -32 under scales of -128 reaches the
    lane sum 8 * 128 * 4 * 32 * 128 = 2^24 exactly and a 64-element item sum twice that, beyond what
    f32 holds exactly; Q3_K with every sc - 32 = -32 and every q - 4 = -4 the lane sum 2^19 and the
    superblock sum 2^22; Q2_K with every scale and min 15 and every q = 3 its largest lane sum and the
    mins product 2 * 15 * 16 * 128; IQ4_XS with every code 0 (-127) and every scale -32 against -127
    the lane sum 8 * 4 * 127 * 127 * 32 = 16 516 096 < 2^24; IQ4_NL 4 * 127 * 127 per block.
    K = 512, N = 8, B = 2."""
    lib, cpu = ref
    T = wt.type
    lo, hi = wt.block(0x00), wt.block(0xFF)
    pairs = [(lo, lo), (hi, hi), (lo, hi), (hi, lo)]
    wq = np.concatenate([np.concatenate(p) for p in pairs + pairs[::-1]])
    K, N, B = 512, 8, 2
    assert wq.size == N * G.row_size(T, K)
    for mk in EXTREME_X:
        x = mk(K)
        yr = G.mul_mat_once(lib, cpu, T, wq, K, N, x, B)
        assert np.abs(yr).max() > 1.0  # the sums did not cancel
        y1 = in_order(rt, 1, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        y0 = in_order(rt, 0, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        assert same_bits(y1, yr), (y1, yr)
        assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)
        if wt.cpy_strict:
            yq = _cpy_then_mul_mat(lib, cpu, wt, wq, K, N, x, B)
            yq1 = in_order(rt, 1, lambda: _cpy_then_mul_mat(rt, backend, wt, wq, K, N, x, B))
            assert same_bits(yq1, yq), (yq1, yq)


def check_default_order_of_a_quantized_chain(rt, backend, ref, wt, B):
    """W1 . x -> RMSNorm -> W2 with the default settings (mmv_order -1): the second mul_mat consumes
    computed activations, so the graph runs in the reference order -- the reference CPU's bits."""
    lib, cpu = ref
    T, K, N1, N2 = wt.type, 1024, 768, 37
    w1, w2 = weights(T, K, N1, 601), weights(T, N1, N2, 602)
    x = synth.uniform(603 + B, K * B)

    def build(L, c):
        a = L.ggml_new_tensor_2d(c, T, K, N1)
        b = L.ggml_new_tensor_2d(c, T, N1, N2)
        xt = L.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, B)
        h = L.ggml_rms_norm(c, L.ggml_mul_mat(c, a, xt), 1e-5)
        return [(a, w1), (b, w2), (xt, x)], L.ggml_mul_mat(c, b, h)

    y = G.graph_once(rt, backend, lambda c: build(rt, c))
    yr = G.graph_once(lib, cpu, lambda c: build(lib, c))
    assert same_bits(y, yr), rel_err(y, yr)


def check_mul_mat_id_top2_of_4_experts(rt, backend, ref, wt, n_tokens):
    """4 experts, the first two ids of every token's row (a strided view), src1 broadcast over the
    ids: decode and a prompt against the reference CPU's MUL_MAT_ID."""
    lib, cpu = ref
    T, K, n, n_as, n_ids = wt.type, 768, 100, 4, 2
    w = weights(T, K, n * n_as, 901)
    x = synth.uniform(902 + n_tokens, K * n_tokens)
    rng = np.random.default_rng(903 + n_tokens)
    ids = np.stack([rng.permutation(n_as) for _ in range(n_tokens)]).astype(np.int32)
    yr = _mul_mat_id(lib, cpu, T, w, K, n, n_as, n_ids, n_tokens, x, ids)
    y1 = in_order(rt, 1, lambda: _mul_mat_id(rt, backend, T, w, K, n, n_as, n_ids, n_tokens, x, ids))
    y0 = in_order(rt, 0, lambda: _mul_mat_id(rt, backend, T, w, K, n, n_as, n_ids, n_tokens, x, ids))
    assert yr.shape == (n * n_ids * n_tokens,) and np.abs(yr).max() > 0
    assert same_bits(y1, yr), rel_err(y1, yr)
    assert rel_err(y0, yr) <= TREE_TOL, rel_err(y0, yr)


def check_quantized_model_file_matches_reference_program(tiny_models, tmp_path, wt):
    import filecmp
    f16, ours = tiny_models[0], tiny_models[1](wt)
    out = str(tmp_path / f"ref-{wt.model}.bin")
    p = subprocess.run([REF_QUANTIZE, f16, out, wt.model], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert os.path.getsize(ours) == os.path.getsize(out)
    assert filecmp.cmp(ours, out, shallow=False)


def check_gpt2_logits_bit_identical_to_reference_cpu(tiny_models, wt, mode):
    """A tiny GPT-2 of the type from quantize_model (its get_rows embedding, its MUL_MAT for every
    projection and the lm_head), default settings: teacher-forced decode, a prompt of more than 8
    tokens in one batch (the chunked > 8 column path) and a prompt in batches of 8 -- the reference
    CPU's logits on the same file, bit for bit."""
    if mode == "decode":
        steps = [[t] for t in TOKENS[:wt.gpt2_decode]]
    elif mode == "batches_of_8":
        steps = [TOKENS[0:8], TOKENS[8:16], TOKENS[16:20]]
    else:
        steps = [TOKENS[:int(mode[len("prompt"):])]]
    ours, rm, free = _both_models(tiny_models[1](wt), max(8, len(steps[0])))
    try:
        assert ours.hp.ftype % 1000 == wt.ftype
        n_past = 0
        for chunk in steps:
            a = ours.eval(n_past, chunk, all_logits=True)
            b = rm.eval(n_past, chunk, all_logits=True)
            assert np.isfinite(b).all() and np.abs(b).max() > 0
            assert same_bits(a, b), (mode, n_past, float(np.mean(a == b)), rel_err(a, b))
            n_past += len(chunk)
    finally:
        free()


def check_split_buffer_weights(rt, backend, wt, B):
    """Rows divided over the slots of a split buffer (slots beyond the device count are virtual
    slots on device 0, each with its own allocation, stream and copies): each slice runs through the
    same mul_mat as the unsplit weight: the unsplit result's bits in the reference order, within
    1e-5 of it in tree order."""
    T, K, N = wt.type, 768, 333  # Q6_K's 630-byte and Q3_K's 330-byte rows: slices start 2 mod 4; IQ4_XS's 408-byte rows: 8 mod 16
    wq = weights(T, K, N, 701)
    x = synth.uniform(702 + B, K * B)
    buft = _split_buft(rt, [1, 1, 0])
    for order in (1, 0):
        def run_split():
            cw = G.Context(rt, rt.ggml_tensor_overhead() * 4, no_alloc=True)
            cx = G.Context(rt, rt.ggml_tensor_overhead() * 8 + rt.ggml_graph_overhead(), no_alloc=True)
            try:
                w = rt.ggml_new_tensor_2d(cw.ctx, T, K, N)
                wbuf = rt.ggml_backend_alloc_ctx_tensors_from_buft(cw.ctx, buft)
                assert wbuf and rt.ggml_backend_buffer_name(wbuf) == b"MI355X_Split"
                xt = rt.ggml_new_tensor_2d(cx.ctx, G.GGML_TYPE_F32, K, B)
                y = rt.ggml_mul_mat(cx.ctx, w, xt)
                g = rt.ggml_new_graph(cx.ctx)
                rt.ggml_build_forward_expand(g, y)
                xbuf = rt.ggml_backend_alloc_ctx_tensors(cx.ctx, backend)
                try:
                    G.tensor_set(rt, w, wq)
                    back = np.empty_like(wq)
                    rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
                    assert np.array_equal(back, wq), "split set/get round trip"
                    G.tensor_set(rt, xt, x)
                    assert rt.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                    return G.tensor_get(rt, y)
                finally:
                    rt.ggml_backend_buffer_free(xbuf)
                    rt.ggml_backend_buffer_free(wbuf)
            finally:
                cx.free()
                cw.free()

        ys = in_order(rt, order, run_split)
        yu = in_order(rt, order, lambda: G.mul_mat_once(rt, backend, T, wq, K, N, x, B))
        if order:
            assert same_bits(ys, yu), rel_err(ys, yu)
        else:
            assert rel_err(ys, yu) <= TREE_TOL, rel_err(ys, yu)


def check_gguf_weights_on_mi355x(rt, backend, tmp_path, family):
    """A GGUF file with a tensor of each type of the family -> MI355X buffer (gguf.Model): the bytes
    arrive, MUL_MAT returns the golden output and, the 32-element types, GET_ROWS the golden
    dequantization."""
    types = rows(family)
    c = types[0].manifest["w"]
    K, N, B = c["K"], c["N"], c["B"]
    wqs = {wt.tag: wt.golden("w.wq.bin") for wt in types}
    path = str(tmp_path / f"{family}.gguf")
    gguf.write(rt, path, [("general.architecture", "str", "test")],
               [("pad", G.GGML_TYPE_F32, [3], np.zeros(3, np.float32))] + [(f"w_{wt.tag}", wt.type, [K, N], wqs[wt.tag]) for wt in types])
    m = gguf.Model(rt, path, backend)
    try:
        x = synth.uniform(c["xseed"], K * B)
        idx = np.array([N - 1, 0, 2, 2], np.int32)
        for wt in types:
            w = m.tensors[f"w_{wt.tag}"]
            assert w.contents.type == wt.type
            back = np.empty(rt.ggml_nbytes(w), np.uint8)
            rt.ggml_backend_tensor_get(w, back.ctypes.data, 0, back.nbytes)
            assert np.array_equal(back, wqs[wt.tag])

            def build_mm(ctx):
                xt = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_F32, K, B)
                return [(xt, x)], rt.ggml_mul_mat(ctx, w, xt)

            def build_gr(ctx):
                i = rt.ggml_new_tensor_1d(ctx, G.GGML_TYPE_I32, len(idx))
                return [(i, idx)], rt.ggml_get_rows(ctx, w, i)

            y = in_order(rt, 1, lambda: G.graph_once(rt, backend, build_mm))
            assert same_bits(y, wt.golden("w.y.f32", np.float32)), wt.tag
            if wt.gguf_get_rows:
                got = G.graph_once(rt, backend, build_gr).reshape(len(idx), K)
                assert same_bits(got, wt.golden("w.wdq.f32", np.float32).reshape(N, K)[idx]), wt.tag
    finally:
        m.free()
