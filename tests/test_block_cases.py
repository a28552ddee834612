"""CPU proofs of tests/block_cases.py: the builders and their inverses, the intended values against
the oracle's dequantizer, the activation rows against the oracle's activation quantizers, every
certificate, the class-E cases bit for bit against the oracle's mul_mat, and, where the reference
library is built, the reference CPU backend's bits on every case of both classes."""
import os

import numpy as np
import pytest

import block_cases as bc
import pyoracle as orc
from ggml_mi355x import ggml as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference lib not built (make -C oracle ref)")

N, B = 70, 8
SIZES = {bc.Q4_K: (256, 1280, 2304), bc.Q5_K: (256, 1280, 2304), bc.Q4_0: (256, 416, 2304), bc.Q8_0: (256, 416, 2304)}
IDS = [c["id"] for c in bc.CASES]


def orc_y(c, K, wq, x, xq):
    t = c["type"]
    return orc.mul_mat(t, wq, K, N, x, B) if c["f32"] else orc.mul_mat_q8(t, wq, K, N, xq, B)


@pytest.mark.parametrize("t", [bc.Q4_0, bc.Q8_0, bc.Q4_K, bc.Q5_K, bc.Q8_K], ids=lambda t: {**bc.NAMES, bc.Q8_K: "q8_K"}[t])
def test_builders_round_trip(t):
    rng = np.random.default_rng(t)
    for _ in range(20):
        d_bits, dmin_bits = (int(v) for v in rng.integers(0, 0x7C00, 2) | rng.integers(0, 2, 2) * 0x8000)
        sc, m = rng.integers(0, 64, 8), rng.integers(0, 64, 8)
        if t == bc.Q4_0:
            f = dict(d_bits=d_bits, q=rng.integers(0, 16, 32))
            blk = bc.q4_0(f["d_bits"], f["q"])
        elif t == bc.Q8_0:
            f = dict(d_bits=d_bits, q=rng.integers(-128, 128, 32))
            blk = bc.q8_0(f["d_bits"], f["q"])
        elif t == bc.Q8_K:
            f = dict(d=float(np.float32(rng.standard_normal())), q=rng.integers(-128, 128, 256))
            blk = bc.q8_K(f["d"], f["q"])
            f["bsums"] = f["q"].reshape(16, 16).sum(1)
        else:
            f = dict(d_bits=d_bits, dmin_bits=dmin_bits, sc=sc, m=m, q=rng.integers(0, bc.QMAX[t] + 1, 256))
            blk = bc.BUILD[t](d_bits, dmin_bits, sc, m, f["q"])
        assert blk.dtype == np.uint8 and blk.size == bc.BYTES[t] == orc.row_size(t, bc.BLCK[t])
        back = bc.parse(t, blk)
        for k, v in f.items():
            assert np.array_equal(back[k], v), (k, back[k], v)
        got = orc.dequantize(t, blk, bc.BLCK[t]).astype(np.float64)
        want = bc.dequantize(t, blk)
        assert np.allclose(got, want, rtol=2.0 ** -22, atol=0), "oracle dequantizer != d * sc * q - dmin * m"


@pytest.mark.parametrize("cid", IDS)
def test_rows_dequantize_to_the_intended_values(cid):
    """orc.dequantize of every hand-made weight row equals d * sc * q - dmin * m exactly (the values
    of the table are short enough for f32 to hold every step)."""
    c = bc.BY_ID[cid]
    t = c["type"]
    K = SIZES[t][-1]
    wq = bc.materialize(cid, K, N, B)[0]
    want = bc.dequantize(t, wq.reshape(-1, bc.BYTES[t])).ravel()
    got = orc.dequantize(t, wq, N * K)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("cid", [c["id"] for c in bc.CASES if c["f32"]])
def test_f32_activations_quantize_to_the_intended_rows(cid):
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in SIZES[t]:
        _, x, xq, _ = bc.materialize(cid, K, N, B)
        assert np.array_equal(orc.quantize_act(bc.ACT[t], x, K), xq), K


@pytest.mark.parametrize("cid", IDS)
def test_certificates_hold(cid):
    c = bc.BY_ID[cid]
    t = c["type"]
    reach = {}
    for K in SIZES[t]:
        ev = bc.materialize(cid, K, N, B)[3]
        if c["cls"] == "E":
            units, u = bc.certificate_E(ev)
            assert units.max() < 2 ** 24, (K, units.max())
            assert u.min() >= -100, (K, u.min())
            assert np.all(np.abs(ev["y"][ev["y"] != 0]) >= 2.0 ** -100)  # normal f32 results
            assert np.count_nonzero(ev["y"]) >= 0.75 * ev["y"].size  # (opposite blocks may cancel to an exact +0)
        else:
            assert np.all(ev["y"] != 0), (K, "a class-S reference output is zero")
            for k in ("T", "U", "pair"):
                if k in ev:
                    reach[k] = max(reach.get(k, 0), int(np.abs(ev[k]).max()))
    if c["cls"] == "S" and not c["f32"]:  # the hand-made rows reach the ends; the F32 constants stop at 127
        want = bc.REACH[t]
        assert {k: reach[k] for k in want} == want, (reach, want)
    if c["cls"] == "S" and c["f32"]:  # (the Q4_0 / Q8_0 ends are +-127 activations already)
        assert reach["T"] == bc.REACH[t]["T"] * (127 if bc.BLCK[t] == 256 else 128) // 128


@pytest.mark.parametrize("cid", [c["id"] for c in bc.CASES if c["cls"] == "E"])
def test_class_E_oracle_returns_the_integer_results_bits(cid):
    c = bc.BY_ID[cid]
    for K in SIZES[c["type"]]:
        wq, x, xq, ev = bc.materialize(cid, K, N, B)
        y = orc_y(c, K, wq, x, xq)
        assert np.array_equal(y.view(np.uint32), bc.expected_bits(ev)), (K, np.flatnonzero(y.view(np.uint32) != bc.expected_bits(ev))[:8])


def mul_mat_src1(lib, backend, t, wq, K, n, src1_type, src1, b):
    def build(c):
        w = lib.ggml_new_tensor_2d(c, t, K, n)
        xt = lib.ggml_new_tensor_2d(c, src1_type, K, b)
        return [(w, wq), (xt, src1)], lib.ggml_mul_mat(c, w, xt)
    return G.graph_once(lib, backend, build)


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


@needs_ref
@pytest.mark.parametrize("cid", IDS)
def test_reference_cpu_returns_the_oracles_bits(ref, cid):
    """The reference CPU backend (AVX2 dot products, F32 or pre-quantized src1 read as it lies) returns
    the oracle's bits on every case of both classes: a case where it does not leaves the table."""
    lib, cpu = ref
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in SIZES[t]:
        wq, x, xq, ev = bc.materialize(cid, K, N, B)
        yr = mul_mat_src1(lib, cpu, t, wq, K, N, G.GGML_TYPE_F32 if c["f32"] else bc.ACT[t], x if c["f32"] else xq, B)
        yo = orc_y(c, K, wq, x, xq)
        bad = np.flatnonzero(yr.view(np.uint32) != yo.view(np.uint32))
        assert bad.size == 0, (K, bad[:8], yr[bad[:4]], yo[bad[:4]])
