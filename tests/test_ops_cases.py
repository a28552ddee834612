"""tests/ops_cases.py on the reference CPU library alone (no GPU): every case computes, builds to the same nodes
on the runtime's core, and the forced/ family cannot pass vacuously. For every forced row or column:

  (a) cpu_order.h's certificate, recomputed from the exact sum with half its margin (the kernel's parallel sum
      is within a quarter of the margin of the exact one), leaves two floats open;
  (b) the reference CPU's value of the compared tensor is what numpy's replay of its arithmetic gives, and
      differs in bits from what the other open float would give -- for k_norm in the F32 output row, for a GEMV
      prologue in the MUL_MAT's output, i.e. after the f16 / q8 rounding of the activations. A row the table
      marks unpinned (ops_cases: pinned False) only has the difference printed; DESIGN.md names those.

The same cases run on MI355X in tests/test_ops_cases_gpu.py."""
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
import ops_cases as OC

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")

pytestmark = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


_reference = {}


def reference(ref, cs):
    if cs.name not in _reference:
        L, cpu = ref
        _reference[cs.name] = OC.run_case(L, cpu, cs, True)[0]
    return _reference[cs.name]


@pytest.mark.parametrize("cs", OC.CASES, ids=repr)
def test_case_on_reference_cpu(ref, cs):
    L, _ = ref
    if cs.expect is not None:
        # the reference CPU aborts on this graph (ops_cases names the assertion): it builds, and numpy's value
        # has the shape and type of the node
        nodes = OC.build_only(L, cs)
        want = cs.expect()["out"]
        assert want.size == int(np.prod(nodes[-1][1])) and not np.isnan(want.astype(np.float32)).any()
        return
    outs = reference(ref, cs)
    for name, v in outs.items():
        assert v.size > 0
        if v.dtype != np.uint8:
            assert not np.isnan(v.astype(np.float32)).any(), f"{name} holds NaN"
    if cs.data and "expect" in cs.data:
        # where the reference does compute an element-wise case, numpy's one IEEE operation is the same bits:
        # this pins the expectation that stands in for the reference on the pairs it aborts on
        assert OC.same_bits(cs.data["expect"]()["out"], outs["out"])


@pytest.mark.parametrize("cs", OC.CASES, ids=repr)
def test_case_builds_the_same_nodes_on_the_runtime(ref, cs):
    """Ops, shapes and op_params in node order: the runtime's builders (ggml_rope_custom among them) and the nodes
    built by hand where it has none make the graph the reference library makes."""
    mine = OC.build_only(G.runtime(), cs)
    theirs = OC.build_only(ref[0], cs, reference=not cs.same_graph)
    assert mine == theirs if cs.same_graph else mine[-1] == theirs[-1]


def straddles(terms):
    lo, hi = OC.certificate(terms, slack=0.5)
    return lo != hi


def check_forced(cs, what, terms, pinned, value, want, alternatives):
    """(a) and (b) for one reduction. value: numpy's replay of the compared tensor; alternatives: other candidate
    float -> the compared tensor with it."""
    assert straddles(terms), f"{what}: the certificate decides this row"
    assert OC.same_bits(value, want), f"{what}: numpy's replay is not the reference CPU's result"
    assert alternatives, f"{what}: no other candidate"
    for o, alt in alternatives.items():
        moved = int(np.sum(alt.view(np.uint32) != want.view(np.uint32)))
        print(f"{cs} {what}: with {float(o).hex()} for the CPU's {float(OC.seq_mean(terms)).hex()}, {moved}/{want.size} elements change")
        if pinned:
            assert moved > 0, f"{what}: the other candidate {float(o).hex()} gives the same bits"


FORCED = OC.by_prefix("forced/")


@pytest.mark.parametrize("cs", FORCED, ids=repr)
def test_forced_rows_are_forced_and_distinguishable(ref, cs):
    L, cpu = ref
    want = reference(ref, cs)["out"]
    assert cs.forced
    if cs.data["kind"] == "k_norm":
        X, rms = cs.data["X"], cs.data["rms"]
        want = want.reshape(X.shape)
        for row, red, pinned in cs.forced:
            x = X[row]
            alts = {o: OC.norm_emul(x, rms, **{red: o}) for o in OC.other_candidates(x, rms, red)}
            check_forced(cs, f"row {row} {red}", OC.reduction_terms(x, rms, red), pinned, OC.norm_emul(x, rms), want[row], alts)
        return
    d = cs.data["gemv"]
    cols = len(d.kinds)
    want = want.reshape(cols, OC.N_ROWS)
    H = np.stack([d.h(c) for c in range(cols)])
    replay = OC.run_case(L, cpu, cs, True, fn=d.fn_given_h(H))[0]["out"].reshape(cols, OC.N_ROWS)
    for c, red, pinned in cs.forced:
        alts = {}
        for o in OC.other_candidates(d.X[c], d.rms, red):
            Ho = H.copy()
            Ho[c] = d.h(c, **{red: o})
            alts[o] = OC.run_case(L, cpu, cs, True, fn=d.fn_given_h(Ho))[0]["out"].reshape(cols, OC.N_ROWS)[c]
        check_forced(cs, f"column {c} {red}", OC.reduction_terms(d.X[c], d.rms, red), pinned, replay[c], want[c], alts)


def test_every_reduction_has_a_pinned_case():
    """Each of cpu_order.h's six fallbacks is forced by a case whose other candidate changes the compared bits:
    the plain sums by a 'mean' entry, the sums of squares by an 'msq' entry, in every family that reaches it."""
    for red, prefixes in OC.REDUCTIONS.items():
        want = "msq" if "<true>" in red else "mean"
        for p in prefixes:
            hits = [c for c in OC.by_prefix(p) if any(r == want and pin for _, r, pin in c.forced)]
            assert hits, (red, p)
    for n in (8, 255, 256, 257, 768, OC.ROW_LDS, OC.ROW_LDS + 1):
        for nn in ("norm", "rms"):
            assert f"forced/k_norm/{nn}-n{n}" in OC.BY_NAME


def test_sum_rows_are_the_rows_of_the_issue():
    """x[0] = n, x[1] = n 2^-24, the rest n 2^-54: the certificate straddles at every length, the CPU's chain
    returns 1.0 (the tie to even), and from n = 768 a 256-lane strided sum returns 1 + 2^-23 -- so there the row
    also catches a replay that walks the elements in another order."""
    for n in (8, 255, 256, 257, 512, 768, 1024, 4096, 12288, 12289):
        x, _ = OC.sum_row(n)
        assert x[0] == n and x[1] == n * 2.0 ** -24 and np.all(x[2:] == np.float32(n * 2.0 ** -54))
        assert straddles(x)
        assert OC.seq_mean(x) == np.float32(1.0)
        lanes = sum(float(np.cumsum(x[l::256].astype(np.float64))[-1]) for l in range(min(n, 256)))
        assert (np.float32(lanes / n) == np.float32(1.0 + 2.0 ** -23)) == (n >= 768), n
        # the big terms at the end: the dust adds up first and lifts the sum over the tie
        assert OC.seq_mean(OC.sum_row(n, 0, "end")[0]) == np.float32(1.0 + 2.0 ** -23)


ROPES = {r.tag(): r for c in OC.by_prefix("rope/") for r in c.data["rope"]}


@pytest.mark.parametrize("tag", sorted(ROPES))
def test_rope_parameters(tag):
    """n_ctx and n_orig_ctx stay within the table's 4096 rows, and with ext_factor != 0 the YaRN ramp lies
    strictly inside the rotated dims, so that some pairs extrapolate, some interpolate and some mix."""
    r = ROPES[tag]
    assert r.n_dims % 2 == 0 and r.n_dims <= r.D and max(OC.ROPE_CTX, r.n_orig) <= OC.ROPE_TABLE
    if r.ext != 0.0:
        lo, hi = r.corr_dims()
        assert 0 < lo < hi < r.n_dims // 2 - 1, (lo, hi)
    assert r.mscale() > 0


def test_rope_table_covers_the_parameter_space():
    rs = list(ROPES.values())
    for mode in (0, 2):
        m = [r for r in rs if r.mode == mode]
        assert {r.D for r in m} == {64, 80, 128}
        assert any(r.n_dims == r.D for r in m) and any(2 * r.n_dims == r.D for r in m) and any((r.D, r.n_dims) == (80, 20) for r in m)
        assert {r.base for r in m} == {10000.0, 500000.0, 1e6} and {r.fs for r in m} == {1.0, 0.25}
        assert {r.ext for r in m} == {0.0, 1.0} and {r.af for r in m} == {1.0, 0.8}
    pos = OC.ROPE_POS
    assert {OC.ROPE_TABLE - 1, OC.ROPE_TABLE} <= set(pos.tolist()) and pos.min() < 0 and pos.max() > 2 * OC.ROPE_TABLE
    assert any(c.replays and c.repeat == 4 and c.launches >= 4 for c in OC.by_prefix("rope/"))
