"""CPU proofs of tests/f16_cases.py: every certificate, the roundings and norm quotients the cases rely
on, the mutants (each wrong kernel, restated in numpy, moves a bit of a named case), and, where the
reference library is built, the reference CPU backend's bits on the graphs tests/f16_graphs.py builds --
the same graphs, fused chains included, that tests/test_f16_cases_gpu.py runs on every F16 route. That pins
the table to the reference, not to the code under test."""
import os
from fractions import Fraction

import numpy as np
import pytest

import f16_cases as fc
import f16_graphs as fg
from ggml_mi355x import ggml as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference lib not built (make -C oracle ref)")

N, B = 70, 8
# K of the GPU runs: one chunk, ragged 128-steps, K % 256 != 0, one / three register passes of the norm
# prologue, the multi-pass ring, the largest K of the fused entry and of the fast path; odd K for the generic GEMV
KS = (8, 136, 1000, 1024, 3072, 4096, 10240, 16384)
KS_NORM = (8, 136, 1000, 1024, 3072)
KS_ODD = (13, 31, 777)


def sizes(cid):
    ks = KS_NORM if cid in fc.NORMS else KS
    return [K for K in ks if fc.fits(cid, K)]


@pytest.mark.parametrize("cid", [c["id"] for c in fc.CASES])
def test_certificates_hold(cid):
    for K in sizes(cid) + [K for K in KS_ODD if fc.fits(cid, K)]:
        m = fc.materialize(cid, K, N, B)
        if m["cls"] == "E":
            units, u = fc.certificate_E(m)
            assert units.max() < 2 ** 24, (K, units.max())
            nz = m["cert_abs"] != 0
            assert u[nz].min() >= -126, (K, u[nz].min())
            assert np.isfinite(m["w16"]).all() == (cid != "E-inf") and np.isinf(m["y"]).any() == (cid == "E-inf")
            assert np.array_equal(m["y"].astype(np.longdouble) if not m.get("gelu") else m["total"].astype(np.float32).astype(np.longdouble),
                                  m["total"]), "the exact result is no f32"
            if "zero" in cid:
                assert np.all(fc.expected_bits(m) == 0), "expected +0.0 everywhere"
            else:
                assert np.count_nonzero(m["y"]) >= 0.55 * m["y"].size
        else:
            assert np.all(np.isfinite(m["y"])) and np.all(m["y"] != 0), (K, "a class-S reference output is zero or not finite")
            assert np.all(np.isfinite(m["xh"].astype(np.float32)))


def test_every_term_counts_in_E_int():
    """Non-zero weights and activations, neighbouring rows and columns different at every k."""
    for K in (8, 1000):
        m = fc.materialize("E-int", K, N, B)
        assert np.all(m["w16"] != 0) and np.all(m["xh"] != 0)
        wi = m["w"] / fc._row_scale(N)[:, None]
        xi = m["x"] / fc._col_scale(B)[:, None]
        assert np.all(wi[1:] != wi[:-1]) and np.all(xi[1:] != xi[:-1])
        assert np.abs(wi).max() <= 8 and np.abs(xi).max() <= 8


def test_onehot_is_a_gather_of_unique_values():
    for K in (8, 136, 1000, 16384):
        m = fc.materialize("E-onehot", K, N, B)
        at = fc.ONEHOT_AT(K)
        for c in range(B):
            assert np.array_equal(m["y"][c], m["w16"][:, at[c % len(at)]].astype(np.float32))
        tile = np.abs(m["w16"][:64, :256].astype(np.float64))
        assert np.unique(tile).size == tile.size


def test_roundings_are_the_known_ones():
    for x, want in fc.ROUND_BIG + [fc.ROUND_MAX] + fc.ROUND_TINY:
        assert np.float64(np.float32(x)) == x, x
        got = fc.rne16(np.float32(x))
        assert got == np.float16(want) and np.signbit(got) == np.signbit(want), (x, got, want)
        assert float(got) != x  # no f16 holds the activation
    m = fc.materialize("E-round", 1000, N, B)
    for v in (2048.0, 2052.0, 65504.0, 2.0 ** -24, 2.0 ** -23):
        assert np.any(m["xh"] == np.float16(v)), v
    assert np.any((m["xh"] == 0) & np.signbit(m["xh"])) and np.any((m["xh"] == 0) & ~np.signbit(m["xh"]))


def test_subnormal_cases_hold_subnormal_operands():
    sub = lambda h: ((h.view(np.uint16) & 0x7C00) == 0) & (h != 0)
    m = fc.materialize("E-subw", 1000, N, B)
    assert np.all(sub(m["w16"])) and np.abs(m["x32"]).min() >= 2.0 ** 10
    assert {1, 0x03FF} <= set(np.unique(m["w16"].view(np.uint16) & 0x7FFF).tolist())
    m = fc.materialize("E-subx", 1000, N, B)
    assert np.all(sub(m["xh"])) and not np.any(sub(m["w16"]))
    assert np.all(m["xh"].astype(np.float32) != m["x32"])


@pytest.mark.parametrize("cid", [c for c in fc.NORMS if c.startswith("E-")])
def test_norm_quotients_are_exact(cid):
    """The mean, the variance (mean square), their quotients by K, the scale and the normalized values and
    their f16 roundings are exact: sequential double sums and f32 tree sums give the same values."""
    for K in sizes(cid):
        m = fc.materialize(cid, K, N, B)
        norm = m["norm"]
        for c in range(B):
            x = [Fraction(float(v)) for v in m["x32"][c]]
            mean = sum(x) / K if norm["mode"] == fc.NORM else Fraction(0)
            assert Fraction(float(np.float32(float(mean)))) == mean
            var = sum((v - mean) ** 2 for v in x) / K
            assert Fraction(float(np.float32(float(var)))) == var
            s2 = var + Fraction(float(np.float32(norm["eps"])))
            p = round(np.log2(float(s2)) / 2)
            assert s2 == Fraction(4) ** p, (cid, K, c, s2)  # a power of four: scale = 2^-p
            scale = Fraction(1, 2 ** p)
            # partial sums of |x| and (x - mean)^2 stay below 2^24 units of the values' lowest bit
            unit = Fraction(2) ** int(fc.odd_exponent(m["x32"][c]).min())
            assert sum(abs(v) for v in x) / unit < 2 ** 24 and sum((v - mean) ** 2 for v in x) / unit ** 2 < 2 ** 24
            h = [(v - mean) * scale for v in x]
            if norm["g"] is not None:
                h = [a * Fraction(float(g)) for a, g in zip(h, norm["g"])]
            if norm["b"] is not None:
                h = [a + Fraction(float(b)) for a, b in zip(h, norm["b"])]
            assert [Fraction(float(v)) for v in m["xh"][c]] == h, (cid, K, c)


# ------------------------------------------------------------------ mutants

def moved(m, y):
    return int(np.count_nonzero(np.ascontiguousarray(y, np.float32).view(np.uint32) != fc.expected_bits(m)))


MUTANTS = [
    # (mutant, the cases it must move, K, N)
    (fc.mutant_drop_last_chunk, ["E-int", "E-onehot", "E-inf", "E-norm-shift-gb"], 136, 70),
    (fc.mutant_last_chunk_not_zeroed, ["E-inf"], 136, 70),
    (fc.mutant_chunk_shift, ["E-int", "E-onehot", "E-subw"], 136, 70),
    (fc.mutant_bias_dropped_on_ragged_rows, ["E-epi-bias", "E-epi-gelu", "E-epi-resid-copies"], 136, 70),
    (fc.mutant_bias_by_row_group, ["E-epi-bias", "E-epi-resid", "E-epi-gelu"], 136, 70),
    (fc.mutant_resid_before_bias, ["S-range-resid"], 136, 70),
    (fc.mutant_mean_over_padded_length, ["E-norm-shift-gb", "E-norm-shift", "E-rms-shift-g", "E-rms-gb"], 136, 70),
    (fc.mutant_flush_subnormals, ["E-subw", "E-subx", "E-round"], 136, 70),
    (fc.mutant_round_toward_zero, ["E-round", "E-subx"], 136, 70),
]


@pytest.mark.parametrize("mutant,cids,K,n", MUTANTS, ids=[mu[0].__name__ for mu in MUTANTS])
def test_mutants_move_the_expected_bits(mutant, cids, K, n):
    for cid in cids:
        m = fc.materialize(cid, K, n, B)
        y = mutant(m)
        if m["cls"] == "E":
            assert moved(m, y) > 0, (mutant.__name__, cid)
        else:  # class S: against the values the reference's node order gives (bias first)
            want = fc._finish(m, m["dot"])
            assert np.count_nonzero(y.view(np.uint32) != want.view(np.uint32)) > 0, (mutant.__name__, cid)
        print(f"{mutant.__name__}: {cid} K={K}: {moved(m, y)} of {y.size} outputs move")


def test_mutants_that_do_not_apply_leave_the_bits():
    """The evaluator of the mutants returns the expected bits when the defect is absent (K a multiple of the
    padded length: the mean over it is the mean)."""
    m = fc.materialize("E-norm-shift-gb", 1024, N, B)
    assert moved(m, fc.mutant_mean_over_padded_length(m)) == 0
    m = fc.materialize("E-epi-resid", 136, 68, B)
    assert moved(m, fc.mutant_bias_dropped_on_ragged_rows(m)) == 0
    assert moved(m, fc.mutant_resid_before_bias(m)) == 0  # exact sums commute: class S holds the order


# ------------------------------------------------------------------ the reference CPU

@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


def same(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.ravel())
    assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:4]], want.ravel()[bad[:4]].view(np.float32))


@needs_ref
@pytest.mark.parametrize("cid", fc.E_IDS)
def test_reference_cpu_returns_the_certificates_bits(ref, cid):
    """Every class-E case on the graphs the GPU runner builds: plain and strided F32 src1, F16 src1 where the
    activations are f16 values, the norm chain, the epilogue nodes and the two row copies; decode and
    prompt column counts; odd K."""
    lib, cpu = ref
    c = fc.BY_ID[cid]
    for K in sizes(cid) + [K for K in KS_ODD if fc.fits(cid, K)]:
        for b in (1, 3, 8) + ((33,) if K in (8, 1024) else ()):
            m = fc.materialize(cid, K, N, b)
            forms = ["f32"] + ([] if c["f32_only"] or m.get("norm") else ["f16"]) + (["strided", "unaligned"] if K % 4 == 0 and K <= 1024 else [])
            for src1 in forms:
                for got, want in zip(fg.run(lib, cpu, m, src1), fg.expected(m)):
                    same(got, want, (cid, K, b, src1))


@needs_ref
@pytest.mark.parametrize("cid", fc.E_IDS)
def test_reference_cpu_on_tall_and_small_matrices(ref, cid):
    """The row counts of the GPU runs: 1, 3, 130 and the tall matrix's 130-row pattern."""
    lib, cpu = ref
    for K in (96, 768):
        if not fc.fits(cid, K):
            continue
        for n in (1, 3, 130):
            m = fc.materialize(cid, K, n, 5)
            for got, want in zip(fg.run(lib, cpu, m), fg.expected(m)):
                same(got, want, (cid, K, n))


@needs_ref
@pytest.mark.parametrize("cid", fc.S_IDS)
def test_reference_cpu_is_within_the_derived_bound_on_class_S(ref, cid):
    """The reference's own summation order obeys the any-order bound the tree-order kernels are held to (and
    its activations are the x^ of the evaluator: the bound's right-hand side is the reference's)."""
    lib, cpu = ref
    for K in sizes(cid):
        m = fc.materialize(cid, K, N, B)
        y = fg.run(lib, cpu, m)[0]
        err = np.abs(y.astype(np.longdouble) - m["total"]).astype(np.float64)
        frac = float((err / fc.tree_bound(m)).max())
        print(f"{cid} K={K}: reference CPU at {frac:.3f} of the bound")
        assert frac <= 1.0, (cid, K, frac)


PARTS = [(H, n_kv, cons) for H in (2, 12, 16) for n_kv in (1, 4, 32)
         for cons in ("E-norm-shift-gb", "E-norm-epi-bias-copies", "E-rms-epi-resid", "E-norm-epi-gelu", None)]


@needs_ref
@pytest.mark.parametrize("H,n_kv,cons", PARTS)
def test_reference_cpu_attention_block_is_exact(ref, H, n_kv, cons):
    """E-parts: with n_kv = 2^p identical K rows the reference's soft_max (fp16 exp table, double sum) gives 2^-p
    for every key, and the block's output and its consumer's are the certificates' bits."""
    lib, cpu = ref
    p = fc.parts_case(H, n_kv, cons, 70)
    assert p["proj_units"].max() < 2 ** 24
    for got, want in zip(fg.run_parts(lib, cpu, p), fg.expected_parts(p)):
        same(got, want, (H, n_kv, cons))


@needs_ref
def test_reference_cpu_on_the_output_over_src1_graph(ref):
    lib, cpu = ref
    m = fg.aliased_case()
    units, u = fc.certificate_E(m)
    assert units.max() < 2 ** 24 and u.min() >= -126
    same(fg.run_aliased(lib, cpu, m), fc.expected_bits(m).reshape(m["B"], m["N"]), "aliased")
