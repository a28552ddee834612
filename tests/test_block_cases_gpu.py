"""The hand-made block cases of tests/block_cases.py on every kernel route of Q4_0 / Q8_0 / Q4_K /
Q5_K. Every test sets its knobs in try / finally, runs the cases and asserts the name of the kernel
the launcher picked (ggml_backend_mi355x_last_mul_mat_route), so that a forced route the shape makes
the launcher ignore fails instead of comparing the default with itself.

Assertions (block_cases.py has the derivations):
  class E: the integer result's bits, on every route, in both orders, prefill included;
  class S, reference order: the oracle's bits (test_block_cases.py pins the oracle to the reference CPU);
  class S, tree order and MFMA: per element |y - exact| <= (n + 3) 2^-24 sum|terms| (block_cases.tree_bound).
The largest observed fraction of that bound per route is printed at the end of the module (pytest -s).
N = 70 rows (68 on the MFMA GEMMs, see NP): ragged row tiles of every kernel; K in {256, 512, 1280, 2304}:
1, 2, 5 and 9 superblocks."""
import contextlib

import numpy as np
import pytest

import block_cases as bc
import pyoracle as orc
from ggml_mi355x import ggml as G

pytestmark = pytest.mark.gpu

N = 70
# The MFMA prefill GEMMs store 16-byte groups: they take dst columns of a 16-byte multiple (N % 4 == 0) and
# leave every other N to the generic GEMV (test_prompt_of_unaligned_columns_takes_the_generic_gemv). 68 rows
# are the closest such size: still ragged in the 16-, 32-, 64- and 128-row tiles.
NP = 68
KS = (256, 512, 1280, 2304)
KQ = (bc.Q4_K, bc.Q5_K)
ALL = [c["id"] for c in bc.CASES]
F32 = [c["id"] for c in bc.CASES if c["f32"]]
KQ_ALL = [c["id"] for c in bc.CASES if c["type"] in KQ]
LEGACY_ALL = [c["id"] for c in bc.CASES if c["type"] not in KQ]
LEGACY_F32 = [c for c in F32 if bc.BY_ID[c]["type"] not in KQ]
DEFAULTS = dict(mmv_order=-1, mmv_variant=0, mmq_variant=0, q40r=1, q80r=1, planes=0, mmqt_short=192, mmid_group=1, mmid_stream=8)
FRACTIONS = {}


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


def src1_of(c, x, xq):
    return (G.GGML_TYPE_F32, x) if c["f32"] else (bc.ACT[c["type"]], xq)


def mul_mat(rt, backend, t, wq, K, n, src1_type, src1, b):
    def build(ctx):
        w = rt.ggml_new_tensor_2d(ctx, t, K, n)
        xt = rt.ggml_new_tensor_2d(ctx, src1_type, K, b)
        return [(w, wq), (xt, src1)], rt.ggml_mul_mat(ctx, w, xt)
    return G.graph_once(rt, backend, build)


def run_case(rt, backend, c, K, B, n=N):
    wq, x, xq, _ = bc.materialize(c["id"], K, n, B)
    return mul_mat(rt, backend, c["type"], wq, K, n, *src1_of(c, x, xq), B)


@pytest.fixture(scope="module")
def oracle_y():
    """The oracle's output of a case at a size, computed once."""
    cache = {}

    def get(c, K, B, n):
        key = (c["id"], K, B, n)
        if key not in cache:
            wq, x, xq, _ = bc.materialize(c["id"], K, n, B)
            t = c["type"]
            cache[key] = orc.mul_mat(t, wq, K, n, x, B) if c["f32"] else orc.mul_mat_q8(t, wq, K, n, xq, B)
        return cache[key]
    return get


def check(c, K, B, y, order, label, oracle_y, sel=None, n=N):
    """y against the case's certificate at n rows; sel: the (column, row) elements y holds (default: all, column-major)."""
    ev = bc.materialize(c["id"], K, n, B)[3]
    pick = (lambda a: a.ravel()) if sel is None else (lambda a: a[sel])
    what = (c["id"], K, B, order, label)
    if c["cls"] == "E":
        want = pick(bc.expected_bits(ev).reshape(B, n))
        bad = np.flatnonzero(y.view(np.uint32) != want)
        assert bad.size == 0, (what, bad[:8], y[bad[:4]], want[bad[:4]].view(np.float32))
    elif order == 1:
        want = pick(oracle_y(c, K, B, n).reshape(B, n))
        bad = np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (what, bad[:8], y[bad[:4]], want[bad[:4]])
    else:
        err = np.abs(y.astype(np.longdouble) - pick(ev["y"])).astype(np.float64)
        bound = pick(bc.tree_bound(c["type"], K, ev))
        frac = float((err / bound).max())
        FRACTIONS[label] = max(FRACTIONS.get(label, 0.0), frac)
        assert frac <= 1.0, (what, frac, int(np.argmax(err / bound)))


def stream_prefix(t):
    return f"k_mmv_stream<type{t},"


def generic_name(t, order):
    return ("k_mmv_kq" if t in KQ else "k_mmv_q0") + ("_ord<" if order else "<")


# ------------------------------------------------------------------ decode

@pytest.mark.parametrize("cid", ALL)
def test_decode_default_kernels(rt, backend, oracle_y, cid):
    """1, 2, 5, 8 columns in both orders: the streaming GEMV for F32 activations (Q4_0 / Q8_0, one
    column, tree order: on the repacked copy), the generic GEMVs k_mmv_kq / k_mmv_q0 (and their
    reference-order replays) for hand-made Q8 rows as src1."""
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in KS:
        for B in (1, 2, 5, 8):
            for order in (0, 1):
                with knobs(rt, mmv_order=order):
                    y = run_case(rt, backend, c, K, B)
                    r = route(rt, backend)
                if c["f32"]:
                    assert r.startswith(stream_prefix(t)) and f",ord{order}," in r, r
                    assert ("repacked," in r) == (t not in KQ and B == 1 and order == 0), r
                    assert f",nc{B if B < 3 else 4 if B < 5 else 8}," in r, r
                else:
                    assert r.startswith(generic_name(t, order)), r
                check(c, K, B, y, order, "decode " + ("k_mmv_stream" if c["f32"] else generic_name(t, order)[:-1]), oracle_y)


def _items(t, K, order, variant, repacked):
    if t in KQ:
        return K // 64
    if t == bc.Q4_0 and order == 0 and (variant % 10 != 1 or repacked):
        return K // 64
    return K // 32


@pytest.mark.parametrize("cid", F32)
def test_decode_mmv_variants(rt, backend, oracle_y, cid):
    """Every mmv_variant value that selects another k_mmv_stream instance: prefetch depth 1, 2, 3 (tens digit;
    rows of more than 64 items: depth 1 or 2 with two items per lane), and for Q4_0 the single-block
    format (ones digit 1) instead of block pairs. q40r / q80r off: the canonical blocks at one column too."""
    c = bc.BY_ID[cid]
    t = c["type"]
    variants = (10, 20, 30) + ((11, 21, 31) if t == bc.Q4_0 else ())
    for K in (512, 2304):
        for B in (1, 5):
            for order in (0, 1):
                for v in variants:
                    with knobs(rt, mmv_order=order, mmv_variant=v, q40r=0, q80r=0):
                        y = run_case(rt, backend, c, K, B)
                        r = route(rt, backend)
                    items = _items(t, K, order, v, False)
                    pd = (1 if v // 10 == 1 else 2) if items > 64 else v // 10
                    assert r.startswith(stream_prefix(t)) and f",pd{pd},ipl{2 if items > 64 else 1}," in r and f",ord{order}," in r, (v, r)
                    assert "repacked," not in r and ("pairs," in r) == (t == bc.Q4_0 and order == 0 and v % 10 != 1), (v, r)
                    check(c, K, B, y, order, "decode k_mmv_stream variants", oracle_y)


@pytest.mark.parametrize("cid", LEGACY_F32)
def test_decode_repacked_copy_on_and_off(rt, backend, oracle_y, cid):
    c = bc.BY_ID[cid]
    t = c["type"]
    knob = "q40r" if t == bc.Q4_0 else "q80r"
    for K in KS:
        for on in (0, 1):
            with knobs(rt, mmv_order=0, **{knob: on}):
                y = run_case(rt, backend, c, K, 1)
                r = route(rt, backend)
            assert r.startswith(stream_prefix(t)) and ("repacked," in r) == bool(on), (on, r)
            check(c, K, 1, y, 0, "decode repacked" if on else "decode canonical blocks", oracle_y)


TALL_N = 16384  # launch_stream: a lone one-column GEMV of at least this many rows of <= 16 items runs four rows per wave step


@pytest.mark.parametrize("cid", [c["id"] for c in bc.CASES if c["f32"] and ("scales" in c["id"] or "bytes" in c["id"] or c["cls"] == "S")])
def test_decode_tall_four_rows_per_step(rt, backend, oracle_y, cid):
    """The smallest N the launcher sends to the MR = 4 form (and one row fewer: the one-row form), the
    case's 70 rows repeated down the matrix."""
    c = bc.BY_ID[cid]
    t, K = c["type"], 256
    wq70, x, xq, ev = bc.materialize(cid, K, N, 1)
    reps = -(-TALL_N // N)
    for n, mr, variant in ((TALL_N, 4, 0), (TALL_N - 1, 1, 0), (TALL_N, 1, 90)):  # (variant 9x: the one-row form asked for)
        wq = np.tile(wq70.reshape(N, -1), (reps, 1))[:n].ravel()
        sel = (np.zeros(n, np.int64), np.arange(n) % N)
        for order in (0, 1):
            with knobs(rt, mmv_order=order, mmv_variant=variant):
                y = mul_mat(rt, backend, t, wq, K, n, G.GGML_TYPE_F32, x, 1)
                r = route(rt, backend)
            assert r.startswith(stream_prefix(t)) and f",mr{mr}," in r, (n, r)
            check(c, K, 1, y, order, f"decode tall mr{mr}", oracle_y, sel)


@pytest.mark.parametrize("cid", LEGACY_ALL)
def test_ragged_k_generic_gemv(rt, backend, oracle_y, cid):
    """Q4_0 / Q8_0 rows of 3 and 13 blocks: the generic GEMVs k_mmv_q0 and k_mmv_q0_ord at decode and prompt column counts."""
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in (96, 416):
        for B in (1, 5, 8, 9, 17):
            for order in (0, 1):
                with knobs(rt, mmv_order=order):
                    y = run_case(rt, backend, c, K, B)
                    r = route(rt, backend)
                assert r.startswith(generic_name(t, order)), r
                check(c, K, B, y, order, "generic " + generic_name(t, order)[:-1], oracle_y)


@pytest.mark.parametrize("cid", F32)
def test_three_members_in_one_decode_launch(rt, backend, oracle_y, cid):
    """Three independent one-column mul_mats of one graph: one grouped k_mmv_stream launch."""
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in (256, 1280):
        wq, x, _, _ = bc.materialize(cid, K, N, 3)
        for order in (0, 1):
            with knobs(rt, mmv_order=order), G.Context(rt, rt.ggml_tensor_overhead() * 16 + rt.ggml_graph_overhead()) as ctx:
                ws = [rt.ggml_new_tensor_2d(ctx.ctx, t, K, N) for _ in range(3)]
                xs = [rt.ggml_new_tensor_2d(ctx.ctx, G.GGML_TYPE_F32, K, 1) for _ in range(3)]
                ys = [rt.ggml_mul_mat(ctx.ctx, w, xt) for w, xt in zip(ws, xs)]
                g = rt.ggml_new_graph(ctx.ctx)
                for yt in ys:
                    rt.ggml_build_forward_expand(g, yt)
                buf = rt.ggml_backend_alloc_ctx_tensors(ctx.ctx, backend)
                assert buf
                try:
                    for i in range(3):
                        G.tensor_set(rt, ws[i], wq)
                        G.tensor_set(rt, xs[i], x[i * K:(i + 1) * K])
                    assert rt.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                    assert rt.ggml_backend_mi355x_last_launch_count(backend) == 1
                    y = np.concatenate([G.tensor_get(rt, yt) for yt in ys])
                    r = route(rt, backend)
                finally:
                    rt.ggml_backend_buffer_free(buf)
            assert r.startswith(stream_prefix(t)) and ",nc1," in r, r
            check(c, K, 3, y, order, "decode grouped k_mmv_stream", oracle_y)


# ------------------------------------------------------------------ prompts

@pytest.mark.parametrize("cid", F32)
def test_reference_order_prompts_in_chunks_of_eight(rt, backend, oracle_y, cid):
    c = bc.BY_ID[cid]
    for K in KS:
        for B in (9, 17):
            with knobs(rt, mmv_order=1):
                y = run_case(rt, backend, c, K, B)
                r = route(rt, backend)
            assert r.startswith(stream_prefix(c["type"])) and ",ord1," in r, r
            check(c, K, B, y, 1, "chunked prompt", oracle_y)


@pytest.mark.parametrize("cid", ALL)
def test_prompt_of_unaligned_columns_takes_the_generic_gemv(rt, backend, oracle_y, cid):
    """N = 70 in tree order: dst columns of 280 bytes, which no MFMA GEMM admits -- whatever mmq_variant asks for,
    the prompt runs on the generic GEMV, eight columns per workgroup."""
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in (256, 2304):
        for B, v in ((9, 0), (17, 128)):
            with knobs(rt, mmv_order=0, mmq_variant=v):
                y = run_case(rt, backend, c, K, B)
                r = route(rt, backend)
            assert r == generic_name(t, 0) + "nc8>", r
            check(c, K, B, y, 0, "prompt on " + generic_name(t, 0)[:-1], oracle_y)


def kq_prefill_route(t, S, B, var):
    """The kernel each mmq_variant value is meant to reach for N = 68 (mi_mul_mat_mmqx_group)."""
    q4 = t == bc.Q4_K
    if var & 128:
        if var & 65536:
            return "k_mmqx_half"
        if var & (1 << 28):
            return "k_mmqx"
        return "k_mmqt" if q4 else "k_mmqw" if S % 4 == 0 else "k_mmqx"
    if B <= 128:
        return "k_mmqp"
    return "k_mmqx_half" if q4 else "k_mmqw" if S % 4 == 0 else "k_mmqx"


KQ_VARIANTS = (128 | 131072, 128 | 65536, 128 | 131072 | (1 << 28))


@pytest.mark.parametrize("cid", KQ_ALL)
def test_prefill_mfma_kernels_k_quants(rt, backend, oracle_y, cid):
    """Tree order, F32 and hand-made Q8_K src1 (the MFMA layout of pre-quantized rows): the default kernel at
    B in {9, 13, 16, 33, 72, 130}, every mmq_variant of test_prefill_kernels_bit_equal at B in {13, 72, 130};
    K = 1024 besides for Q5_K's k_mmqw (superblock counts that are multiples of 4)."""
    c = bc.BY_ID[cid]
    t = c["type"]
    runs = [(K, B, 0) for K in KS for B in (9, 13, 16, 33, 72, 130)]
    runs += [(K, B, v) for K in KS for B in (13, 72, 130) for v in KQ_VARIANTS]
    if t == bc.Q5_K:
        runs += [(1024, 130, 0), (1024, 72, 128 | 131072)]
    for K, B, v in runs:
        with knobs(rt, mmv_order=0, mmq_variant=v):
            y = run_case(rt, backend, c, K, B, NP)
            r = route(rt, backend)
        assert r == kq_prefill_route(t, K // 256, B, v), (K, B, v, r)
        check(c, K, B, y, 0, "prefill " + r, oracle_y, n=NP)


LEGACY_VARIANTS = {0: "k_mmq0p", 16: "k_mmq0p", 128: "k_mmq0x_rows2", 128 | 65536: "k_mmq0x_half", 128 | (1 << 24): "k_mmq0x_rows2",
                   128 | (1 << 25): "k_mmq0x_rows2_w8"}


@pytest.mark.parametrize("cid", LEGACY_ALL)
def test_prefill_mfma_kernels_q4_0_q8_0(rt, backend, oracle_y, cid):
    c = bc.BY_ID[cid]
    runs = [(K, B, 0) for K in KS for B in (9, 13, 16, 33, 72, 130)]
    runs += [(K, B, v) for K in KS for B in (13, 72, 130) for v in LEGACY_VARIANTS if v]
    for K, B, v in runs:
        with knobs(rt, mmv_order=0, mmq_variant=v):
            y = run_case(rt, backend, c, K, B, NP)
            r = route(rt, backend)
        assert r == LEGACY_VARIANTS[v], (K, B, v, r)
        check(c, K, B, y, 0, "prefill " + r, oracle_y, n=NP)


@pytest.mark.parametrize("cid", [c for c in KQ_ALL if bc.BY_ID[c]["type"] == bc.Q4_K])
def test_prefill_repacked_planes(rt, backend, oracle_y, cid):
    """planes 1: Q4_K prompts of more than 128 columns on k_mmqr."""
    c = bc.BY_ID[cid]
    for K in KS:
        with knobs(rt, mmv_order=0, planes=1):
            y = run_case(rt, backend, c, K, 130, NP)
            r = route(rt, backend)
        assert r == "k_mmqr", r
        check(c, K, 130, y, 0, "prefill k_mmqr", oracle_y, n=NP)


def _two_members(rt, backend, c, K, B, host=False):
    """Two independent prompts of one graph (the same weights, the case's columns and the same columns in
    reverse order); host: one member alone whose output lies in the host buffer type."""
    t = c["type"]
    wq, x, xq, _ = bc.materialize(c["id"], K, NP, B)
    st, src = src1_of(c, x, xq)
    rev = np.ascontiguousarray(src.reshape(B, -1)[::-1]).ravel()
    ovh = rt.ggml_tensor_overhead() * 16 + rt.ggml_graph_overhead()
    with G.Context(rt, ovh) as cd, G.Context(rt, ovh) as ch:
        n = 1 if host else 2
        ws = [rt.ggml_new_tensor_2d(cd.ctx, t, K, NP) for _ in range(n)]
        xs = [rt.ggml_new_tensor_2d(cd.ctx, st, K, B) for _ in range(n)]
        ys = [rt.ggml_mul_mat(ch.ctx if host else cd.ctx, w, xt) for w, xt in zip(ws, xs)]
        g = rt.ggml_new_graph(ch.ctx if host else cd.ctx)
        for yt in ys:
            rt.ggml_build_forward_expand(g, yt)
        bufs = [rt.ggml_backend_alloc_ctx_tensors(cd.ctx, backend)]
        if host:
            bufs.append(rt.ggml_backend_alloc_ctx_tensors_from_buft(ch.ctx, rt.ggml_backend_mi355x_host_buffer_type()))
        assert all(bufs)
        try:
            for w, xt, s in zip(ws, xs, (src, rev)):
                G.tensor_set(rt, w, wq)
                G.tensor_set(rt, xt, s)
            assert rt.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            launches = rt.ggml_backend_mi355x_last_launch_count(backend)
            outs = [G.tensor_get(rt, yt) for yt in ys]
            return outs, launches, route(rt, backend)
        finally:
            for b in bufs[::-1]:
                rt.ggml_backend_buffer_free(b)


@pytest.mark.parametrize("cid", [c for c in ALL if bc.BY_ID[c]["f32"]])
def test_prefill_grouped_launch_of_two(rt, backend, oracle_y, cid):
    """Two prompts as one quantizer launch and one grouped GEMM launch; Q4_K with mmqt_short 1 besides: k_mmqt's short form."""
    c = bc.BY_ID[cid]
    t = c["type"]
    for K in (512, 2304):
        for short in ((192, 1) if t == bc.Q4_K else (192,)):
            B = 72
            with knobs(rt, mmv_order=0, mmqt_short=short):
                (y0, y1), launches, r = _two_members(rt, backend, c, K, B)
            assert launches == 2, launches
            assert r == ("k_mmqt_short" if short == 1 else "k_mmqp" if t in KQ else "k_mmq0p"), r
            check(c, K, B, y0, 0, "prefill grouped " + r, oracle_y, n=NP)
            check(c, K, B, np.ascontiguousarray(y1.reshape(B, NP)[::-1]).ravel(), 0, "prefill grouped " + r, oracle_y, n=NP)


@pytest.mark.parametrize("cid", KQ_ALL)
def test_prefill_long_prompt_into_host_memory(rt, backend, oracle_y, cid):
    """More than 128 columns with the output in the host buffer type: the kernel that stores each element once."""
    c = bc.BY_ID[cid]
    for K in (256, 2304):
        with knobs(rt, mmv_order=0):
            (y,), _, r = _two_members(rt, backend, c, K, 130, host=True)
        assert r == "k_mmqp", r
        check(c, K, 130, y, 0, "prefill host output k_mmqp", oracle_y, n=NP)


# ------------------------------------------------------------------ MUL_MAT_ID

@pytest.mark.parametrize("cid", F32)
def test_mul_mat_id_streaming_and_grouped(rt, backend, oracle_y, cid):
    """Three experts of 70 rows each (rows 70 e .. 70 e + 69 of the case at 210 rows), two ids per token: the
    streaming decode form (a k_mmv_stream member per pair), pair by pair on the generic GEMV, and the
    pairs grouped by expert (mmid_group 4), each expert's rows class-E (or class-S) rows of their own."""
    c = bc.BY_ID[cid]
    t = c["type"]
    n_as, n_ids, n_tok = 3, 2, 5
    ids = np.array([[(tk + e) % n_as for e in range(n_as)] for tk in range(n_tok)], np.int32)
    for K in (256, 1280):
        wq, x, _, ev = bc.materialize(cid, K, N * n_as, n_tok)
        want_sel = (np.repeat(np.arange(n_tok), n_ids * N),
                    (ids[:, :n_ids, None] * N + np.arange(N)).ravel())

        def build(ctx):
            a = rt.ggml_new_tensor_3d(ctx, t, K, N, n_as)
            b = rt.ggml_new_tensor_3d(ctx, G.GGML_TYPE_F32, K, 1, n_tok)
            full = rt.ggml_new_tensor_2d(ctx, G.GGML_TYPE_I32, n_as, n_tok)
            top = rt.ggml_view_2d(ctx, full, n_ids, n_tok, full.contents.nb[1], 0)
            return [(a, wq), (b, x), (full, ids)], rt.ggml_mul_mat_id(ctx, a, b, top)

        for label, kv, name in (("stream", dict(), None), ("pairs", dict(mmid_stream=0, mmid_group=0), "id_pairs"),
                                ("grouped", dict(mmid_stream=0, mmid_group=4), "nc4,id_grouped")):
            for order in (0, 1):
                with knobs(rt, mmv_order=order, **kv):
                    y = G.graph_once(rt, backend, build)
                    r = route(rt, backend)
                if name is None:
                    assert r.startswith(stream_prefix(t)) and r.endswith(",ids1>") and f",ord{order}," in r, r
                else:
                    assert r.startswith(generic_name(t, order)) and name in r, r
                _check_rows(c, K, N * n_as, n_tok, y, order, "mul_mat_id " + label, want_sel, ev)


def _check_rows(c, K, n_rows, B, y, order, label, sel, ev):
    """check() for a materialization of n_rows rows (the experts of a MUL_MAT_ID)."""
    what = (c["id"], K, B, order, label)
    if c["cls"] == "E":
        want = bc.expected_bits(ev).reshape(B, n_rows)[sel]
        bad = np.flatnonzero(y.view(np.uint32) != want)
        assert bad.size == 0, (what, bad[:8], y[bad[:4]], want[bad[:4]].view(np.float32))
        return
    wq, x, _, _ = bc.materialize(c["id"], K, n_rows, B)
    if order == 1:
        want = orc.mul_mat(c["type"], wq, K, n_rows, x, B).reshape(B, n_rows)[sel]
        bad = np.flatnonzero(y.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (what, bad[:8], y[bad[:4]], want[bad[:4]])
        return
    err = np.abs(y.astype(np.longdouble) - ev["y"][sel]).astype(np.float64)
    bound = bc.tree_bound(c["type"], K, ev)[sel]
    frac = float((err / bound).max())
    FRACTIONS[label] = max(FRACTIONS.get(label, 0.0), frac)
    assert frac <= 1.0, (what, frac)
