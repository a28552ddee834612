"""What the BF16 tests share (tests/test_bf16.py, test_bf16_gpu.py, golden/make_bf16_golden.py): the
converter's input set, the MUL_MAT cases with their seeded inputs, and a numpy
restatement of the reference's ggml_vec_dot_bf16 (AVX2 build) whose steps can be swapped for the
mutants a wrong kernel would compute.
"""
import functools
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN
from ggml_mi355x import ggml as G

BF16 = G.GGML_TYPE_BF16



@functools.lru_cache(maxsize=None)
def manifest():
    """tests/golden/bf16.json (written by tests/golden/make_bf16_golden.py from the reference library)."""
    with open(os.path.join(GOLDEN, "bf16.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ the converter's input set

LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)


@functools.lru_cache(maxsize=None)
def converter_set():
    """Every upper-16-bit pattern x the six lower halves: 393 216 f32 values (as uint32 bits)."""
    u = (np.arange(65536, dtype=np.uint32)[:, None] << 16) | np.array(LOW_HALVES, np.uint32)[None, :]
    u = u.ravel()
    u.setflags(write=False)
    return u


def converter_classes(u):
    """How many members of the set fall in each class the reference converter treats on its own."""
    mag, low = u & 0x7fffffff, u & 0xffff
    exp, man = (u >> 23) & 0xff, u & 0x7fffff
    finite = (exp != 0) & (exp != 0xff)
    return {
        "pos_zero": int((u == 0).sum()),
        "neg_zero": int((u == 0x80000000).sum()),
        "subnormal": int(((exp == 0) & (man != 0)).sum()),               # flushed to a signed zero
        "subnormal_neg": int(((exp == 0) & (man != 0) & (u >> 31 == 1)).sum()),
        "tie_to_even_down": int((finite & (low == 0x8000) & ((u >> 16) & 1 == 0)).sum()),  # exactly half, even upper half: stays
        "tie_to_even_up": int((finite & (low == 0x8000) & ((u >> 16) & 1 == 1)).sum()),    # exactly half, odd upper half: up
        "below_half": int((finite & (low == 0x7fff)).sum()),
        "above_half": int((finite & (low == 0x8001)).sum()),
        "carry_to_inf": int(((mag >= 0x7f7f8000) & (mag < 0x7f800000)).sum()),       # 0x7f7fffff and friends round to inf
        "inf": int((mag == 0x7f800000).sum()),
        "quiet_nan": int(((mag > 0x7f800000) & (u & 0x400000 != 0)).sum()),
        "signalling_nan": int(((mag > 0x7f800000) & (u & 0x400000 == 0)).sum()),
        "nan_payload_low_half_only": int(((mag > 0x7f800000) & (u & 0x7f0000 == 0)).sum()),  # (bits >> 16) alone would read as inf
        "nan_payload_high_half_only": int(((mag > 0x7f800000) & (low == 0)).sum()),
    }


def converter_sample(u):
    """The members whose reference outputs are committed as bf16_convert_sample.u16: every zero, subnormal,
    inf and NaN of the set and every 61st of the rest (the full set's outputs are pinned by their SHA-256)."""
    exp = (u >> 23) & 0xff
    keep = (exp == 0) | (exp == 0xff)
    keep[::61] = True
    return np.flatnonzero(keep)


def f16_patterns_as_f32(lib):
    """All 65 536 f16 bit patterns converted to f32 by lib (exact). (The reference converts through a table
    that its ggml_init fills: a context is made first.)"""
    h = np.arange(65536, dtype=np.uint16)
    out = np.empty(65536, np.float32)
    with G.Context(lib, lib.ggml_tensor_overhead() * 2, no_alloc=True):
        lib.ggml_fp16_to_fp32_row(h.ctypes.data, out.ctypes.data, 65536)
    assert out[0x3c00] == 1.0
    return out


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ the MUL_MAT cases

# (K, N, B): a sparse cross of K in {8, 32, 33, 40, 100, 256, 1000, 1001, 4096, 4104} (leftovers only; one
# step; odd K, rows 2-byte aligned; leftovers of 8, 4 and 1; long rows with and without a tail), N in
# {1, 5, 67} and B in {1, 2, 3, 5, 8, 9, 17, 33, 130} with every value of each axis at least once, the pairs
# K 1001 x B 9 and K 4104 x B 130, B 33 and 130 at N 67 (ragged 32 x 32 tiles in both directions, more
# than 128 columns), and K 64 and 320 at B 17 (fewer 64-deep K chunks than waves; a count the 4 waves
# do not divide).
CASES = ((8, 5, 1), (32, 1, 2), (33, 67, 3), (40, 5, 5), (100, 67, 8), (256, 67, 33), (1000, 1, 17), (1001, 5, 9),
         (4096, 67, 1), (4104, 67, 130), (64, 5, 17), (320, 67, 17))
CASE_IDS = [f"K{K}-N{N}-B{B}" for K, N, B in CASES]
GOLDEN_CASES = ((33, 67, 3), (100, 67, 8), (1001, 5, 9))  # their reference outputs are committed
SUBNORMAL_AT = 3  # element of every activation column that holds an f32 subnormal
# Seeds, searched once (the first of 0, 1, 2, ... that works) so that every mutant of MUTANTS that applies to
# the case's K changes at least one output bit (test_bf16.py asserts it): sums of a few 16-bit products
# are often exact in f32, so in the small cases not every stream tells the orders apart.
SEEDS = {(8, 5, 1): 87, (32, 1, 2): 1}


def to_bf16(x):
    return G.f32_to_bf16(np.asarray(x, np.float32))


@functools.lru_cache(maxsize=None)
def case_inputs(K, N, B, seed=None):
    """(w bf16 bits [N, K], x f32 [B, K]). Normal weights and uniform activations, except element
    SUBNORMAL_AT: every column holds an f32 subnormal there (the reference flushes it to a signed zero)
    against weights of 2^126, so that a converter that keeps subnormals moves every output by ~0.25."""
    rng = np.random.default_rng([7000, K, N, B, SEEDS.get((K, N, B), 0) if seed is None else seed])
    w = rng.standard_normal((N, K)).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, (B, K)).astype(np.float32)
    w[:, SUBNORMAL_AT] = np.where(rng.integers(0, 2, N) == 1, 2.0 ** 126, -(2.0 ** 126)).astype(np.float32)
    x[:, SUBNORMAL_AT] = (rng.integers(0x00180000, 0x007fffff, B).astype(np.uint32)
                          | (rng.integers(0, 2, B).astype(np.uint32) << 31)).view(np.float32)
    wb = to_bf16(w)
    wb.setflags(write=False)
    x.setflags(write=False)
    return wb, x


def weight_bytes(wb):
    return np.ascontiguousarray(wb, np.uint16).view(np.uint8).ravel()


# ------------------------------------------------------------------ ggml_vec_dot_bf16 in numpy

def _trunc_bf16(x):
    return (np.asarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _keep_subnormals_bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    rne = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return np.where((u & 0x7fffffff) > 0x7f800000, (u >> 16) | 64, rne).astype(np.uint16)


MUTANTS = ("truncate", "keep_subnormals", "f32_activations", "sequential_sum", "f32_leftovers")


def mul_mat_numpy(wb, x, mutant=None):
    """MUL_MAT(w bf16 [N, K], x f32 [B, K]) -> [B, N] as the reference's AVX2 build computes it: x rounded
    with ggml_fp32_to_bf16_row; per step of 32 the lane sums c_r[j] = fma(w, x, c_r[j]) (the product of two
    bf16 values is exact in f32, so a rounded add of it is the fma); (c1 + c3) + (c2 + c4); upper + lower
    half; g + movehl(g); lane 0 + lane 1; to double; the K % 32 leftovers added one by one as doubles of
    f32 products; cast to float. `mutant` swaps one step for what a wrong kernel would do."""
    assert mutant is None or mutant in MUTANTS
    w = G.bf16_to_f32(wb).reshape(wb.shape)
    if mutant == "f32_activations":
        xa = np.asarray(x, np.float32)
    else:
        conv = {"truncate": _trunc_bf16, "keep_subnormals": _keep_subnormals_bf16}.get(mutant, to_bf16)
        xa = G.bf16_to_f32(conv(x)).reshape(x.shape)
    N, K = w.shape
    B = xa.shape[0]
    np_ = K & ~31

    def fma(a, b, c):  # exact for bf16 operands; for the f32-activation mutant the double product is exact, one extra rounding
        return (c.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32) if mutant == "f32_activations" \
            else c + a * b

    with np.errstate(all="ignore"):
        if mutant == "sequential_sum":
            s = np.zeros((B, N), np.float32)
            for i in range(K):
                s = fma(xa[:, None, i], w[None, :, i], s)
            return s
        acc = np.zeros((B, N, 32), np.float32)
        for i in range(0, np_, 32):
            acc = fma(xa[:, None, i:i + 32], w[None, :, i:i + 32], acc)
        c = acc.reshape(B, N, 4, 8)
        v = (c[:, :, 0] + c[:, :, 2]) + (c[:, :, 1] + c[:, :, 3])
        g = v[:, :, 4:] + v[:, :, :4]
        g = g[:, :, :2] + g[:, :, 2:]
        r = g[:, :, 0] + g[:, :, 1]
        if mutant == "f32_leftovers":
            s = r
            for i in range(np_, K):
                s = s + xa[:, None, i] * w[None, :, i]
            return s
        s = r.astype(np.float64)
        for i in range(np_, K):
            s = s + (xa[:, None, i] * w[None, :, i]).astype(np.float64)
        return s.astype(np.float32)


def mutant_applies(mutant, K):
    """Where a mutant can change a bit at all. The lane order needs a 32-step (K >= 32). Leftovers in f32
    need two of them: with one, the double sum of two floats is exact and rounds once, as the f32 add does.
    The three converter mutants apply everywhere."""
    if mutant == "sequential_sum":
        return K >= 32
    if mutant == "f32_leftovers":
        return K % 32 >= 2
    return True
