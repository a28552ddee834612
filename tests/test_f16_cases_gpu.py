"""The hand-made F16 cases of tests/f16_cases.py on every F16 mul_mat route. Every test sets its knobs in
try / finally, runs the cases and asserts the route string the launcher recorded
(ggml_backend_mi355x_last_mul_mat_route), so that a forced route the shape makes the launcher ignore fails
instead of comparing the default with itself. The expected route of the tree-order decode GEMVs is
fast_route() below: the dispatch of mi_mul_mat_f16_fast restated, from which the shapes were derived
(DESIGN 4.11 has the table).

Assertions (f16_cases.py has the derivations):
  class E: the exact result's bits, on every route, in both orders, fused or not, prompts included;
  class S, reference order: the reference CPU's bits (the same graph on oracle/_ref/libggml_ref.so);
  class S, tree order and MFMA: per element |y - exact| <= gamma(K) sum|w x^| (f16_cases.tree_bound).
The largest observed fraction of that bound per route and the routes asserted are printed at the end of the
module (pytest -s)."""
import contextlib
import os

import numpy as np
import pytest

import f16_cases as fc
import f16_graphs as fg
from ggml_mi355x import ggml as G

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")

N = 70        # ragged in the 4-, 16-, 32- and 64-row groups
NP = 68       # the MFMA prompt GEMMs store 16-byte groups: N % 4 == 0
TALL = 16385  # (N + 3) / 4 >= 4096 row groups: the grid-stride kernels; one row past a multiple of 4 and of 16
TALL_PATTERN = 130
DEFAULTS = dict(mmv_order=-1, f16_variant=0, f16_threads=0, f16_waves=0, f16_rgs=0, f16_ps_waves=0, f16_norm_waves=0, f16_nc=10,
                f16_bn=5, f16_mt=1)
FRACTIONS, ROUTES, UNCOMPARED = {}, {}, []
PLAIN_E = [c for c in fc.PLAIN if c.startswith("E-")]
PLAIN_S = [c for c in fc.PLAIN if c.startswith("S-")]
NORM_E = [c for c in fc.NORMS if c.startswith("E-")]
NORM_S = [c for c in fc.NORMS if c.startswith("S-")]
NO_EPI = ["E-int", "E-onehot", "E-inf", "E-round", "E-subw", "E-subx", "E-zero"]


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def backend(rt):
    b = G.mi355x_backend(rt, 0)
    yield b
    rt.ggml_backend_free(b)
    for k in sorted(FRACTIONS):
        print(f"\nlargest fraction of the derived bound, {k}: {FRACTIONS[k]:.3f}", end="")
    for k in sorted(ROUTES):
        print(f"\nroute asserted {ROUTES[k]:5d} x {k}", end="")
    if UNCOMPARED:
        print(f"\n{UNCOMPARED[0]} class-S reference-order runs not compared: the reference library is not built", end="")
    print()


@contextlib.contextmanager
def knobs(rt, **kv):
    try:
        for k, v in kv.items():
            assert rt.ggml_backend_mi355x_set_tuning(k.encode(), v), (k, v)
        yield
    finally:
        for k in kv:
            rt.ggml_backend_mi355x_set_tuning(k.encode(), DEFAULTS[k])


def route(rt, backend):
    return rt.ggml_backend_mi355x_last_mul_mat_route(backend).decode()


def epi_of(m, tall=False):
    if m.get("gelu"):
        return 3
    if m["resid"] is not None and not tall:
        return 2
    return 1 if m["bias"] is not None else 0


def _u(per):
    return 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8


def fast_route(m, f16_waves=0, f16_rgs=0, f16_nc=10, f16_bn=5, f16_mt=1, f16_norm_waves=0, **_):
    """mi_mul_mat_f16_fast's decision for the case's shape (not the summed-partials prologue)."""
    K, n, B = m["K"], m["N"], m["B"]
    norm = m.get("norm") is not None and m["norm"]["g"] is not None  # (a norm without mul(g) is no prologue)
    epi = epi_of(m)
    kp = -(-K // 128) * 128
    nit = kp // 128
    nc = 8 if B >= 8 else 4 if B >= 3 else B
    while nc > 1 and nc * kp * 2 > 60000:
        nc //= 2
    cap = f16_nc // 10 if norm else f16_nc % 10
    if cap > 0 and (n + 3) // 4 < 4096:
        while nc > 1 and nc > cap:
            nc //= 2
    chunks = -(-B // nc)
    groups = (n + 3) // 4 * chunks
    want = f16_waves if f16_waves > 0 else (768 if norm else 2048)
    ks = max(1, min(8, want // max(groups, 1)))
    ks = min(ks, nit)
    if norm:
        ks = max(ks, (nit + 7) // 8)
    if norm and nc > 1:
        ks = max(ks, min(f16_norm_waves if f16_norm_waves > 0 else 3, nit))
    per = -(-nit // ks)
    ks = -(-nit // per)
    rgs = max(1, min(f16_rgs, 8 // ks)) if f16_rgs > 0 else 1
    two_copies = len(m.get("copies") or []) > 1
    if (n + 3) // 4 >= 4096 and K <= 1024 and m["resid"] is None and not two_copies and f16_rgs == 0 and (B == 1 or B == nc):
        jm, te = (4 if norm else 0), epi_of(m, tall=True)
        if nc >= 2 and B >= 2 and K % 32 == 0 and K <= 768 and f16_mt:
            return f"k_gemv_f16_mt<jm{jm},nk24,epi{te}>"
        return f"k_gemv_f16_tall<nc{nc},u8,jm{jm},epi{te}>"
    if norm and (B > 1 or f16_bn >= 10) and K <= 1024 and f16_bn > 0:
        bn = f16_bn % 10
        nw, kss = (16 if bn == 5 else 8 if bn >= 2 else 4), (2 if bn == 3 else 4 if bn >= 4 else 1)
        return f"k_gemv_f16_bn<nw{nw},ks{kss},epi{epi}>"
    if norm:
        return f"k_gemv_f16<nc{nc},u{_u(per)},one,jm{4 if K <= 1024 else 12},epi{epi},xh0>[ks{ks},rgs{rgs}]"
    if per <= 8:
        return f"k_gemv_f16<nc{nc},u{_u(per)},one,jm0,epi{epi},xh0>[ks{ks},rgs{rgs}]"
    return f"k_gemv_f16<nc{nc},u8,ring,jm0,epi{epi},xh0>[ks{ks},rgs{rgs}]"


def ordered_route(m, f16_variant=0, f16_threads=0, **_):
    """launch_f16_x's decision (mmv_order 1, and tree order where the fast path refuses the operands)."""
    K, n, B = m["K"], m["N"], m["B"]
    norm = m.get("norm") is not None and m["norm"]["g"] is not None
    nc = min(B, 4, max((32768 - (2 * K if norm else 0)) // K, 1))
    chunks = -(-B // nc)
    if f16_variant == 0 and K >= 32 and n * chunks < 16384:
        return f"k_mmv_f16_w16<nc{nc},ks{48 if K <= 3072 else 16},epi{epi_of(m)}>[t{f16_threads or 256}]"
    return f"k_mmv_f16_x<nc{nc},u{32 if n * chunks <= 8192 else 8},epi{epi_of(m)}>[t{256 if n >= 16384 else 64}]"


class Run:
    """Runs cases, collects every mismatch of a test and raises them together at the end."""

    def __init__(self, rt, backend, ref=None):
        self.rt, self.backend, self.ref, self.bad, self.n = rt, backend, ref, [], 0

    def case(self, m, want_route, order=0, src1="f32", label=None, **kn):
        with knobs(self.rt, mmv_order=order, **kn):
            outs, r = fg.run(self.rt, self.backend, m, src1, after=route)
        what = (m["id"], m["K"], m["N"], m["B"], f"order{order}", src1, kn)
        self.n += 1
        ok = want_route(r) if callable(want_route) else r == want_route
        if not ok:
            self.bad.append((what, "route", r, None if callable(want_route) else want_route))
        ROUTES[r] = ROUTES.get(r, 0) + 1
        self.check(m, outs, order, label or r.split("<")[0], what, src1)
        return r

    def check(self, m, outs, order, label, what, src1="f32"):
        if m["cls"] == "E":
            for i, (got, want) in enumerate(zip(outs, fg.expected(m))):
                bad = np.flatnonzero(got.view(np.uint32).ravel() != want.ravel())
                if bad.size:
                    self.bad.append((what, f"output {i}: {bad.size} of {want.size} differ, first at (col, row) "
                                     f"{[divmod(int(b), want.shape[1]) for b in bad[:4]]}", got.ravel()[bad[:4]], want.ravel()[bad[:4]].view(np.float32)))
        elif order == 1:
            if self.ref is None:
                UNCOMPARED[:] = [(UNCOMPARED[0] if UNCOMPARED else 0) + 1]
                return
            want = fg.run(self.ref[0], self.ref[1], m, src1)
            for i, (got, w) in enumerate(zip(outs, want)):
                bad = np.flatnonzero(got.view(np.uint32).ravel() != w.view(np.uint32).ravel())
                if bad.size:
                    self.bad.append((what, f"output {i}: {bad.size} differ from the reference CPU", got.ravel()[bad[:4]], w.ravel()[bad[:4]]))
        else:
            err = np.abs(outs[0].astype(np.longdouble) - m["total"]).astype(np.float64)
            frac = float((err / fc.tree_bound(m)).max())
            FRACTIONS[label] = max(FRACTIONS.get(label, 0.0), frac)
            if not frac <= 1.0:
                self.bad.append((what, f"{frac:.3f} of the derived bound", int(np.argmax(err / fc.tree_bound(m)))))

    def done(self):
        assert not self.bad, f"{len(self.bad)} mismatches in {self.n} runs; first: " + "\n".join(repr(b) for b in self.bad[:6])


def tall(cid, K, B, copies=None):
    return fc.tile_rows(fc.materialize(cid, K, TALL_PATTERN, B), TALL, copies)


# ------------------------------------------------------------------ tree-order decode: k_gemv_f16

@pytest.mark.parametrize("cid", fc.PLAIN)
def test_plain_gemv_columns(rt, backend, cid):
    """1, 2, 3, 5, 7, 8 columns (NC 1 / 2 / 4 / 8 with ragged last column groups) at K = 8 .. 3072: one step per wave
    (u1) up to K = 1024, u4 on 8 waves at K = 3072; N = 70."""
    run = Run(rt, backend)
    for K in (8, 136, 1000, 1024, 3072):
        if not fc.fits(cid, K):
            continue
        for B in (1, 2, 3, 5, 7, 8):
            m = fc.materialize(cid, K, N, B)
            run.case(m, fast_route(m))
    run.done()


@pytest.mark.parametrize("cid", fc.PLAIN)
def test_lds_fallback_of_columns_and_long_rows(rt, backend, cid):
    """K = 4096 with 8 columns: 64 KB of f16 columns do not fit, four per workgroup; K = 10240, the longest row the fused
    entry (mi_mul_mat_f16_fused_supported) admits: two per workgroup and the two-deep ring of 8-step batches (10 steps
    per wave). K = 16384 is within mi_mul_mat_f16_fast_supported but never gets there: the generic k_mmv_f16_ord runs
    it, so the one-column-per-workgroup end of the fallback (K > 15000) is reached by no shape."""
    run = Run(rt, backend)
    for K, B, nc, form in ((4096, 8, 4, "u4,one"), (4096, 5, 4, "u4,one"), (10240, 8, 2, "u8,ring"), (10240, 1, 1, "u8,ring"), (10240, 3, 2, "u8,ring")):
        m = fc.materialize(cid, K, N, B)
        r = run.case(m, fast_route(m))
        assert f"<nc{nc},{form}," in r, r
    for B in (1, 8):
        m = fc.materialize(cid, 16384, N, B)
        run.case(m, f"k_mmv_f16_ord<nc{min(B, 4)},aligned1,id0>", label="K = 16384 on the generic k_mmv_f16_ord")
    run.done()


@pytest.mark.parametrize("cid", fc.PLAIN)
def test_steps_per_wave_and_the_ring(rt, backend, cid):
    """f16_waves 1: one wave per row group, so K sets the steps per wave: u2 (K = 136), u4 (512), u8 (1000), and from
    K = 1152 (9 steps) the multi-pass ring; f16_waves 36: two waves of four steps each at K = 1000."""
    run = Run(rt, backend)
    for K, form in ((136, "u2,one"), (512, "u4,one"), (1000, "u8,one"), (1152, "u8,ring"), (3072, "u8,ring")):
        if not fc.fits(cid, K):
            continue
        for B in (1, 2, 3, 8):
            m = fc.materialize(cid, K, N, B)
            r = run.case(m, fast_route(m, f16_waves=1), f16_waves=1)
            assert f",{form}," in r and "[ks1," in r, r
    if fc.fits(cid, 1000):
        m = fc.materialize(cid, 1000, N, 1)
        r = run.case(m, fast_route(m, f16_waves=36), f16_waves=36)
        assert ",u4,one," in r and "[ks2," in r, r
    run.done()


@pytest.mark.parametrize("cid", fc.PLAIN)
def test_row_groups_per_workgroup(rt, backend, cid):
    """f16_rgs 2 and 8 (with one wave per row group): 8 and 32 rows per workgroup, ragged at N = 70 and 130."""
    run = Run(rt, backend)
    for K in (136, 1000):
        if not fc.fits(cid, K):
            continue
        for n in (N, 130):
            for B in (1, 8):
                for rgs in (2, 8):
                    m = fc.materialize(cid, K, n, B)
                    r = run.case(m, fast_route(m, f16_waves=1, f16_rgs=rgs), f16_waves=1, f16_rgs=rgs)
                    assert r.endswith(f"[ks1,rgs{rgs}]"), r
    run.done()


@pytest.mark.parametrize("cid", fc.PLAIN)
def test_columns_per_workgroup_cap(rt, backend, cid):
    """f16_nc's ones digit 0 / 1 / 2 / 4 with 8 and 5 columns."""
    run = Run(rt, backend)
    for K in (136, 1000):
        if not fc.fits(cid, K):
            continue
        for B in (8, 5):
            for cap in (0, 1, 2, 4):
                m = fc.materialize(cid, K, N, B)
                r = run.case(m, fast_route(m, f16_nc=10 + cap), f16_nc=10 + cap)
                assert f"<nc{min(cap or 8, 8 if B == 8 else 4)}," in r, r
    run.done()


@pytest.mark.parametrize("cid", fc.PLAIN + fc.NORMS)
def test_row_counts_and_epilogues(rt, backend, cid):
    """N in {1, 3, 70, 130} (ragged in the 4-, 16- and 64-row groups) at one and five columns, every epilogue,
    the two row copies; norm cases on their default kernels (k_gemv_f16 jm4 / jm12, k_gemv_f16_bn)."""
    run = Run(rt, backend)
    for K in (8, 136, 1000, 3072):
        if not fc.fits(cid, K):
            continue
        for n in (1, 3, 130):
            for B in (1, 5):
                m = fc.materialize(cid, K, n, B)
                run.case(m, fast_route(m))
    run.done()


# ------------------------------------------------------------------ tree-order decode: the norm prologue

@pytest.mark.parametrize("cid", fc.NORMS)
def test_norm_prologue_one_column(rt, backend, cid):
    """One column: K <= 1024 in four registers per lane (jm4), 1024 < K <= 3072 in twelve (jm12), each wave its own
    normalized copy; f16_bn 11 - 15: the one column on k_gemv_f16_bn."""
    run = Run(rt, backend)
    for K, jm in ((8, 4), (136, 4), (512, 4), (1000, 4), (1024, 4), (1032, 12), (3072, 12)):
        m = fc.materialize(cid, K, N, 1)
        r = run.case(m, fast_route(m))
        if m["norm"]["g"] is not None:
            assert r.startswith("k_gemv_f16<nc1,") and f",jm{jm}," in r, r
        else:
            assert ",jm0," in r, r  # a norm alone runs as its own kernel in front of a plain GEMV
        if K in (136, 1000, 3072) and m["norm"]["g"] is not None:  # one wave per row group: u2 / u8 with jm4, three waves of u8 with jm12
            r = run.case(m, fast_route(m, f16_waves=1), f16_waves=1)
            assert f",u{2 if K == 136 else 8},one,jm{jm}," in r, r
        if K == 512 and m["norm"]["g"] is not None:
            r = run.case(m, fast_route(m, f16_waves=1), f16_waves=1)
            assert f",u4,one,jm4," in r, r
        if K <= 1024 and m["norm"]["g"] is not None:
            for bn in (11, 12, 13, 14, 15):
                r = run.case(m, fast_route(m, f16_bn=bn), f16_bn=bn)
                assert r.startswith("k_gemv_f16_bn<"), r
    run.done()


@pytest.mark.parametrize("cid", [c for c in fc.NORMS if c != "E-norm-shift"])
def test_norm_prologue_several_columns(rt, backend, cid):
    """2, 5, 8 columns: f16_bn 1 - 5 (k_gemv_f16_bn: 4 / 8 / 16 waves, K split over 1 / 2 / 4 waves); f16_bn 0: k_gemv_f16 with
    f16_nc's tens digit 1 / 2 / 4 / 8 columns per workgroup and f16_norm_waves 1 / 3; K > 1024: k_gemv_f16 jm12."""
    run = Run(rt, backend)
    for K in (8, 136, 1000, 1024):
        for B in (2, 5, 8):
            m = fc.materialize(cid, K, N, B)
            for bn in (1, 2, 3, 4, 5):
                r = run.case(m, fast_route(m, f16_bn=bn), f16_bn=bn)
                assert r.startswith("k_gemv_f16_bn<"), r
    for K in (136, 1000, 3072):
        for B in (2, 5, 8):
            m = fc.materialize(cid, K, N, B)
            for tens in (1, 2, 4, 8):
                for nw in (1, 3):
                    kn = dict(f16_bn=0, f16_nc=10 * tens, f16_norm_waves=nw)
                    r = run.case(m, fast_route(m, **kn), **kn)
                    assert r.startswith("k_gemv_f16<") and f",jm{4 if K <= 1024 else 12}," in r, r
    m = fc.materialize(cid, 3072, N, 5)
    r = run.case(m, fast_route(m))
    assert r.startswith("k_gemv_f16<nc1,") and ",jm12," in r, r
    run.done()


# ------------------------------------------------------------------ tree-order decode: tall matrices

TALL_CASES = ["E-int", "E-onehot", "E-inf", "E-zero", "E-subw", "E-subx", "E-round", "E-epi-bias", "E-epi-gelu", "E-norm-gb", "E-norm-shift-gb",
              "E-rms-shift-g", "E-norm-epi-gelu", "S-range", "S-range-norm"]


@pytest.mark.parametrize("cid", TALL_CASES)
def test_tall_matrices(rt, backend, cid):
    """N = 16385: k_gemv_f16_tall with NC 1 / 2 / 4 / 8 (f16_mt 0 for several columns), k_gemv_f16_mt for 2 / 4 / 8
    columns at K % 32 == 0; 3 and 5 columns stay on k_gemv_f16; K = 32, 96 (ragged 128-step) and 768; epilogues none,
    bias, GELU and one row copy."""
    run = Run(rt, backend)
    for K, cols in ((32, (1, 2, 3, 4, 8)), (96, (1, 2, 5, 8)), (768, (1, 8))):
        if not fc.fits(cid, K) or (K == 768 and cid in ("E-onehot", "E-zero", "E-subx", "E-round", "E-rms-shift-g")):
            continue
        for B in cols:
            m = tall(cid, K, B)
            for mt in ((1, 0) if B in (2, 4, 8) else (1,)):
                r = run.case(m, fast_route(m, f16_mt=mt), f16_mt=mt)
                if B in (3, 5):  # no whole column group: the row-group kernels (k_gemv_f16, with the norm prologue k_gemv_f16_bn)
                    assert r.startswith(("k_gemv_f16<", "k_gemv_f16_bn<")), r
                else:
                    assert r.startswith("k_gemv_f16_mt<" if mt and B > 1 else f"k_gemv_f16_tall<nc{B},"), r
    if cid in ("E-epi-bias", "E-epi-gelu", "E-norm-epi-gelu"):
        for B in (1, 4):  # one CPY of a row range (the logits into a staging tensor): stored by the tall kernels
            m = tall(cid, 96, B, copies=[(5, 16001)])
            for mt in (1, 0):
                r = run.case(m, fast_route(m, f16_mt=mt), f16_mt=mt)
                assert r.startswith("k_gemv_f16_mt<" if mt and B > 1 else "k_gemv_f16_tall<"), r
    run.done()


# ------------------------------------------------------------------ tree-order decode: src1 layouts

@pytest.mark.parametrize("cid", fc.PLAIN + fc.NORMS)
def test_src1_layouts(rt, backend, ref_or_none, cid):
    """A strided view with 16-byte-aligned columns stays on the fast path; a view whose columns are only 4-byte
    aligned leaves it for the reference-order kernel k_mmv_f16_w16 (whatever mmv_order says); an F16 src1 runs on
    the generic k_mmv_f16_ord."""
    run = Run(rt, backend, ref_or_none)
    c = fc.BY_ID[cid]
    for K in (136, 1000):
        for B in (1, 5):
            m = fc.materialize(cid, K, N, B)
            run.case(m, fast_route(m), src1="strided")
            prologue = m.get("norm") is not None and m["norm"]["g"] is not None
            if m.get("norm") is None or prologue:
                r = run.case(m, ordered_route(m), order=0, src1="unaligned", label="unaligned src1 on k_mmv_f16_w16")
                assert r.startswith("k_mmv_f16_w16<"), r
            if not c["f32_only"] and m.get("norm") is None:
                r = run.case(m, lambda r: r.startswith("k_mmv_f16_ord<"), src1="f16")
                assert r == f"k_mmv_f16_ord<nc{min(B, 4)},aligned1,id0>", r
    run.done()


@pytest.fixture(scope="module")
def ref_or_none():
    if not os.path.exists(REF_LIB):
        yield None
        return
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


def test_output_over_src1_takes_the_converted_copy(rt, backend):
    """The output (added in place into the residual) overlaps src1: the columns are first converted into scratch and the
    GEMV reads those f16 columns (XH), in tree order and in the reference's."""
    m = fg.aliased_case()
    want = fc.expected_bits(m).reshape(m["B"], m["N"])
    for order, name in ((0, "k_gemv_f16<nc4,u1,one,jm0,epi2,xh1>[ks2,rgs1]"), (1, "k_mmv_f16_w16<nc3,ks48,epi2>[t256]")):
        with knobs(rt, mmv_order=order):
            y, r = fg.run_aliased(rt, backend, m, after=route)
        ROUTES[r] = ROUTES.get(r, 0) + 1
        assert r == name, r
        bad = np.flatnonzero(y.view(np.uint32).ravel() != want.ravel())
        assert bad.size == 0, (order, bad[:8], y.ravel()[bad[:4]], want.ravel()[bad[:4]].view(np.float32))


# ------------------------------------------------------------------ tree-order decode: summed partials (E-parts)

PS = [(H, n_kv, cons) for H in (2, 16) for n_kv in (1, 4) for cons in ("E-norm-shift-gb", "E-norm-epi-bias-copies", "E-rms-epi-resid", "E-norm-epi-gelu")]
PS += [(12, 4, "E-norm-epi-gelu"), (12, 1, "E-rms-epi-resid")]  # GPT-2's own shape: 12 parts, K = 768 (QPT 2 with two waves)


@pytest.mark.parametrize("H,n_kv,cons", PS)
def test_attention_block_into_summed_partials_gemv(rt, backend, H, n_kv, cons):
    """E-parts: k_attn_proj leaves c_proj's output as H per-head partial sums; the LN -> F16 GEMV consumer adds them
    in its prologue (k_gemv_f16_ps: NPM 12 for H = 2 and 12, 16 for H = 16; f16_ps_waves 2 / 4 / 8: QPT 2 at K = 768 and 1024 with
    two waves) and its first workgroup stores the block's output. Four epilogues, F = 70 rows."""
    bad = []
    p = fc.parts_case(H, n_kv, cons, N)
    epi = epi_of(p["consumer"])
    for rw in (0, 2, 4, 8):
        with knobs(rt, mmv_order=0, f16_ps_waves=rw):
            outs, r = fg.run_parts(rt, backend, p, after=route)
        qpt = 2 if (p["E"] // 4 + 64 * (rw or 4) - 1) // (64 * (rw or 4)) > 1 else 1
        want = f"k_gemv_f16_ps<npm{12 if H <= 12 else 16},qpt{qpt},epi{epi}>[rw{rw or 4}]"
        ROUTES[r] = ROUTES.get(r, 0) + 1
        if r != want:
            bad.append((rw, "route", r, want))
        for name, got, w in zip(("y", "O"), outs, fg.expected_parts(p)):
            d = np.flatnonzero(got.view(np.uint32) != w)
            if d.size:
                bad.append((rw, name, d.size, d[:4], got[d[:4]], w[d[:4]].view(np.float32)))
    assert not bad, bad


@pytest.mark.parametrize("H,n_kv", [(2, 1), (2, 4), (16, 1), (16, 32)])
def test_attention_block_with_another_consumer_sums_the_partials(rt, backend, H, n_kv):
    """The same block consumed by add(O, O): mi_sum_parts stores O first; no F16 GEMV follows, so the last recorded
    route is not a summed-partials GEMV's."""
    p = fc.parts_case(H, n_kv, None, N)
    with knobs(rt, mmv_order=0):
        _, marker = fg.run(rt, backend, fc.materialize("E-int", 8, 1, 1), after=route)
        outs, r = fg.run_parts(rt, backend, p, after=route)
    assert marker.startswith("k_gemv_f16<") and r == marker, (r, marker)  # c_proj ran inside k_attn_proj: no mul_mat route since
    for name, got, w in zip(("y", "O"), outs, fg.expected_parts(p)):
        d = np.flatnonzero(got.view(np.uint32) != w)
        assert d.size == 0, (name, d.size, d[:4], got[d[:4]], w[d[:4]].view(np.float32))


# ------------------------------------------------------------------ reference-order decode

@pytest.mark.parametrize("cid", fc.PLAIN + fc.NORMS)
def test_reference_order_decode(rt, backend, ref_or_none, cid):
    """mmv_order 1: k_mmv_f16_w16 with kS 48 (K <= 3072) and 16 (K = 4096), f16_threads 64 / 128 / 256; f16_variant 1: the
    quad-per-row k_mmv_f16_x with U = 32. Class S: the reference CPU's bits (skipped where its library is not built)."""
    run = Run(rt, backend, ref_or_none)
    norm = cid in fc.NORMS
    for K in (8, 136, 1000, 3072) + (() if norm else (4096,)):
        if not fc.fits(cid, K):
            continue
        for B in (1, 2, 3, 5, 8):
            m = fc.materialize(cid, K, N, B)
            r = run.case(m, ordered_route(m), order=1)
            assert r.startswith("k_mmv_f16_w16<" if K >= 32 else "k_mmv_f16_x<"), r
            if B in (1, 5) and K in (136, 3072, 4096):
                for t in (64, 128):
                    run.case(m, ordered_route(m, f16_threads=t), order=1, f16_threads=t)
            if B in (1, 2, 5):
                r = run.case(m, ordered_route(m, f16_variant=1), order=1, f16_variant=1)
                assert r.startswith("k_mmv_f16_x<") and ",u32," in r, r
    run.done()


@pytest.mark.parametrize("cid", ["E-int", "E-onehot", "E-inf", "E-zero", "E-subw", "E-epi-bias", "E-epi-gelu", "E-norm-shift-gb", "S-range"])
def test_reference_order_tall(rt, backend, ref_or_none, cid):
    """N = 16385 in reference order: the quad kernel by default, U = 8 (more than 8192 rows) in 256-thread workgroups."""
    run = Run(rt, backend, ref_or_none)
    for K, B in ((96, 1), (96, 3), (32, 8)):
        if cid == "S-range" and B > 1:
            continue
        m = tall(cid, K, B)
        r = run.case(m, ordered_route(m), order=1)
        assert r.startswith("k_mmv_f16_x<") and ",u8," in r and r.endswith("[t256]"), r
    run.done()


# ------------------------------------------------------------------ the generic GEMV

@pytest.mark.parametrize("cid", [c for c in PLAIN_E + PLAIN_S if not fc.BY_ID[c]["needs"] > 1])
def test_generic_gemv_odd_k(rt, backend, ref_or_none, cid):
    """K % 8 != 0: no fused kernel takes it; k_mmv_f16_ord (unaligned rows), 1 - 4 columns per workgroup, in both orders."""
    run = Run(rt, backend, ref_or_none)
    for K in (13, 31, 777):
        for B in (1, 2, 3, 5):
            for order in (0, 1):
                m = fc.materialize(cid, K, N, B)
                run.case(m, f"k_mmv_f16_ord<nc{min(B, 4)},aligned0,id0>", order=order, label="generic k_mmv_f16_ord")
    run.done()


def test_generic_gemv_weight_batches_and_broadcast(rt, backend):
    """Weights [K, N, 2], src1 [K, B, 4] (each weight batch serves two src1 batches), F32 and F16 src1: batch i of the
    weights holds the case's rows rotated by i, batch j of src1 its columns rotated by j."""
    bad = []
    for cid, K, src_f16 in (("E-int", 136, False), ("E-int", 13, False), ("E-int", 136, True), ("E-subw", 136, True), ("E-onehot", 136, False)):
        for B in (1, 2, 3, 5):
            m = fc.materialize(cid, K, N, B)
            want = fc.expected_bits(m).reshape(B, N)
            w = np.stack([np.roll(m["w16"], -i, axis=0) for i in range(2)])
            x = np.stack([np.roll(m["xh"] if src_f16 else m["x32"], -j, axis=0) for j in range(4)])

            def build(c):
                wt = rt.ggml_new_tensor_3d(c, G.GGML_TYPE_F16, K, N, 2)
                xt = rt.ggml_new_tensor_3d(c, G.GGML_TYPE_F16 if src_f16 else G.GGML_TYPE_F32, K, B, 4)
                return [(wt, w), (xt, x)], rt.ggml_mul_mat(c, wt, xt)
            with knobs(rt, mmv_order=0):
                y = G.graph_once(rt, backend, build).reshape(4, B, N)
                r = route(rt, backend)
            ROUTES[r] = ROUTES.get(r, 0) + 1
            if r != f"k_mmv_f16_ord<nc{min(B, 4)},aligned{int(K % 8 == 0)},id0>":
                bad.append((cid, K, B, "route", r))
            for j in range(4):
                e = np.roll(np.roll(want, -j, axis=0), -(j // 2), axis=1)
                if not np.array_equal(y[j].view(np.uint32), e):
                    bad.append((cid, K, B, src_f16, "batch", j))
    assert not bad, bad


def test_mul_mat_id_pair_by_pair(rt, backend):
    """MUL_MAT_ID of F16 experts: three experts of 70 rows (rows 70 e .. 70 e + 69 of the case at 210 rows), two ids per
    token, on the generic kernel pair by pair, in both orders."""
    n_as, n_ids, n_tok = 3, 2, 5
    ids = np.array([[(tk + e) % n_as for e in range(n_as)] for tk in range(n_tok)], np.int32)
    for cid, K in (("E-int", 136), ("E-int", 13), ("E-subw", 1000), ("E-inf", 136)):
        m = fc.materialize(cid, K, N * n_as, n_tok)
        sel = (np.repeat(np.arange(n_tok), n_ids * N), (ids[:, :n_ids, None] * N + np.arange(N)).ravel())
        want = fc.expected_bits(m).reshape(n_tok, N * n_as)[sel]

        def build(c):
            a = rt.ggml_new_tensor_3d(c, G.GGML_TYPE_F16, K, N, n_as)
            b = rt.ggml_new_tensor_3d(c, G.GGML_TYPE_F32, K, 1, n_tok)
            full = rt.ggml_new_tensor_2d(c, G.GGML_TYPE_I32, n_as, n_tok)
            top = rt.ggml_view_2d(c, full, n_ids, n_tok, full.contents.nb[1], 0)
            return [(a, m["w16"]), (b, m["x32"]), (full, ids)], rt.ggml_mul_mat_id(c, a, b, top)
        for order in (0, 1):
            with knobs(rt, mmv_order=order):
                y = G.graph_once(rt, backend, build)
                r = route(rt, backend)
            ROUTES[r] = ROUTES.get(r, 0) + 1
            assert r == f"k_mmv_f16_ord<nc1,aligned{int(K % 8 == 0)},id1>", r
            bad = np.flatnonzero(y.view(np.uint32) != want)
            assert bad.size == 0, (cid, K, order, bad[:8], y[bad[:4]], want[bad[:4]].view(np.float32))


# ------------------------------------------------------------------ prompts

PROMPT_CASES = NO_EPI + ["E-epi-bias", "E-epi-gelu", "S-range"]


def mmq3_route(K):
    if K % 512:
        return "k_mmq3<sk1,nst0>"
    return f"k_mmq3<sk2,nst{K // 128 if K // 128 in (16, 24, 32) else 0}>"


@pytest.mark.parametrize("cid", PROMPT_CASES)
def test_prompt_gemms(rt, backend, cid):
    """k_mmf16p at 9, 32, 33 and 128 columns; k_mmq3 at 129 and 257: K = 256, 1280 (SK 1), 512, 6144 (SK 2, runtime
    stage count), 2048 / 3072 / 4096 (SK 2 unrolled over 16 / 24 / 32 stages); N = 68 and 4; K = 8192 at N = 68."""
    run = Run(rt, backend)
    for K in (256, 512, 1280, 2048, 3072, 4096, 6144):
        for n in (NP, 4):
            for B in ((9, 33, 129) if K not in (256, 4096) else (9, 32, 33, 128, 129, 257)):
                if n == 4 and B not in (9, 129):
                    continue
                m = fc.materialize(cid, K, n, B)
                run.case(m, "k_mmf16p<pf3>" if B <= 128 else mmq3_route(K))
    for B in (33, 129):
        m = fc.materialize(cid, 8192, NP, B)
        run.case(m, "k_mmf16p<pf3>" if B <= 128 else "k_mmq3<sk2,nst0>")
    run.done()


@pytest.mark.parametrize("cid", PROMPT_CASES)
def test_prompts_the_gemms_refuse(rt, backend, ref_or_none, cid):
    """K % 256 != 0 and N % 4 != 0 (dst columns of no 16-byte multiple): the prompt runs on the generic GEMV, four columns
    per workgroup, in the reference's order."""
    run = Run(rt, backend, ref_or_none)
    for K, n in ((136, NP), (1000, NP), (256, N), (1280, N)):
        for B in (9, 33):
            m = fc.materialize(cid, K, n, B)
            run.case(m, "k_mmv_f16_ord<nc4,aligned1,id0>", label="prompt on the generic k_mmv_f16_ord")
    run.done()


# ------------------------------------------------------------------ a replayed capture

def test_replayed_capture_of_fused_chains(rt, backend):
    """Four fused chains in one graph (ln -> c_attn + bias + copies, ln -> c_fc + bias + GELU, mul_mat + bias + residual +
    copies, rms -> mul_mat + residual): computed four times -- launched, captured, replayed twice -- every compute gives
    the certificates' bits."""
    import ctypes
    ms = [fc.materialize(cid, 1000, N, 1) for cid in ("E-norm-epi-bias-copies", "E-norm-epi-gelu", "E-epi-resid-copies", "E-rms-epi-resid")]
    be = G.mi355x_backend(rt, 0)

    def stats():
        arr = (ctypes.c_int64 * 6)()
        assert rt.ggml_backend_mi355x_graph_stats_ex(be, arr, 6) == 6
        return list(arr)
    try:
        overhead = rt.ggml_tensor_overhead() * 160 + rt.ggml_graph_overhead()
        with knobs(rt, mmv_order=0), G.Context(rt, overhead, no_alloc=True) as ctx:
            built = [fg.build(rt, ctx.ctx, m) for m in ms]
            g = rt.ggml_new_graph(ctx.ctx)
            for feeds, outs, extra in built:
                rt.ggml_build_forward_expand(g, outs[0])
                for e in extra:
                    rt.ggml_build_forward_expand(g, e)
            buf = rt.ggml_backend_alloc_ctx_tensors(ctx.ctx, be)
            assert buf
            try:
                for feeds, _, _ in built:
                    for t, arr in feeds:
                        G.tensor_set(rt, t, arr)
                s0 = stats()
                for it in range(4):
                    assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
                    assert rt.ggml_backend_mi355x_last_launch_count(be) == 4, "one launch per fused chain"
                    for m, (_, outs, _) in zip(ms, built):
                        for o, want in zip(outs, fg.expected(m)):
                            got = G.tensor_get(rt, o)
                            assert np.array_equal(got.view(np.uint32), want.ravel()), (it, m["id"])
                    for o in [o for _, outs, _ in built for o in outs]:  # the next compute must write them again
                        G.tensor_set(rt, o, np.full(rt.ggml_nbytes(o) // 4, np.nan, np.float32))
                s1 = stats()
                assert s1[4] - s0[4] == 2, ("two replays expected", s0, s1)
            finally:
                rt.ggml_backend_buffer_free(buf)
    finally:
        rt.ggml_backend_free(be)
