"""Companion ops (csrc/kernels/ops.hip) and the norm prologues of the decode GEMVs (mmv_ordered.hip,
mmv_fused_impl.h), shared by tests/test_ops_cases.py (reference CPU alone: the preconditions) and
tests/test_ops_cases_gpu.py (MI355X against the reference CPU).

A case is a graph `fn(b) -> outs` (name -> tensor, expanded in that order) through any library exporting the
ggml API, as in fusion_cases.py. Three families:

  forced/   rows whose mean (or mean of squares) sits on a float rounding midpoint, so that cpu_order.h's
            certificate cannot decide them and the kernel replays the CPU's sequential double chain. Every
            such row is listed in `cs.forced` with the reduction it forces; tests/test_ops_cases.py proves
            that the certificate straddles and that the other candidate float would change the compared tensor.
  rope/     ggml_rope_custom over its parameter space, positions inside, at the edge of and outside the
            backend's host-built table.
  layout/   permuted, broadcast, strided and in-place operands, type pairs, row lengths around kRowLds.

Everything is compared bit for bit with the reference CPU, except RoPE positions outside the table (a derived
bound, rope_bound) and the few element-wise type pairs the reference CPU aborts on, whose expected value is one
IEEE operation in numpy (`cs.expect`).
"""
import ctypes
import math

import numpy as np

from ggml_mi355x import ggml as G
import fusion_cases as FC
from fusion_cases import new, op_name, same_bits, u

F32, F16, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32
Q4_0, Q8_0, Q8_1, Q4_K, Q5_K, Q8_K = G.GGML_TYPE_Q4_0, G.GGML_TYPE_Q8_0, G.GGML_TYPE_Q8_1, G.GGML_TYPE_Q4_K, G.GGML_TYPE_Q5_K, G.GGML_TYPE_Q8_K
TYPE_NAME = {F32: "f32", F16: "f16", Q8_0: "q8_0", Q8_1: "q8_1", Q4_K: "q4_K", Q5_K: "q5_K", Q8_K: "q8_K"}
NP_TYPE = {F32: np.float32, F16: np.float16, I32: np.int32}

EPS = 1e-5
ROW_LDS = 12288  # kRowLds: k_norm / k_soft_max stage longer rows in the dst row
f32 = np.float32


def p2(e):
    return math.ldexp(1.0, e)


# ------------------------------------------------------------------ cases and running them

class Builder:
    """What a case's graph function gets. `reference`: the graph is being built for the reference CPU (a few
    layouts its forwards assert against are made contiguous there first: the values are the same)."""

    def __init__(self, L, c, reference):
        self.L, self.c, self.reference = L, c, reference
        self.feeds = []

    def leaf(self, arr, *ne, ttype=F32):
        t = new(self.L, self.c, ttype, *ne)
        self.feeds.append((t, np.ascontiguousarray(arr)))
        return t


class Case:
    """expect: () -> name -> array where the reference CPU cannot compute the graph. check: (name, got, want) ->
    list of complaints, where the comparison is not identical bits. launches: the backend's launch count.
    orders: the mmv_order settings the case runs under (None: the default). repeat: computes of the one graph.
    forced: [(column or row, reduction, pinned)] for the forced/ family."""

    def __init__(self, name, fn, expect=None, check=None, launches=None, orders=(None,), repeat=1, forced=(), data=None,
                 n_tensors=48, replays=False, same_graph=True):
        self.name, self.fn, self.expect, self.check, self.launches = name, fn, expect, check, launches
        self.orders, self.repeat, self.forced, self.data, self.n_tensors, self.replays = orders, repeat, list(forced), data, n_tensors, replays
        self.same_graph = same_graph  # False: the reference CPU gets another graph of the same values (Builder.reference)

    def __repr__(self):
        return self.name


CASES = []


def add(name, fn, **kw):
    CASES.append(Case(name, fn, **kw))
    return CASES[-1]


def by_prefix(prefix):
    return [c for c in CASES if c.name.startswith(prefix)]


def read(L, t):
    """A tensor's values; the raw bytes of a quantized one."""
    return G.tensor_get(L, t, NP_TYPE.get(t.contents.type, np.uint8))


def run_case(L, backend, cs, reference, fn=None):
    """Builds `cs` (or another graph function with the same data) with every tensor in storage of its own,
    computes it cs.repeat times and returns name -> values and the backend's last launch count."""
    with G.Context(L, L.ggml_tensor_overhead() * cs.n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
        b = Builder(L, c.ctx, reference)
        outs = (fn or cs.fn)(b)
        g = L.ggml_new_graph(c.ctx)
        for t in outs.values():
            L.ggml_build_forward_expand(g, t)
        buf = L.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in b.feeds:
                G.tensor_set(L, t, arr)
            for _ in range(cs.repeat):
                assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            n = L.ggml_backend_mi355x_last_launch_count(backend) if L.has("ggml_backend_mi355x_last_launch_count") else 0
            return {k: read(L, t) for k, t in outs.items()}, n
        finally:
            L.ggml_backend_buffer_free(buf)


def build_only(L, cs, reference=False):
    """The case's graph on a library without computing it: ops, shapes and parameters in node order."""
    with G.Context(L, L.ggml_tensor_overhead() * cs.n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
        outs = cs.fn(Builder(L, c.ctx, reference))
        g = L.ggml_new_graph(c.ctx)
        for t in outs.values():
            L.ggml_build_forward_expand(g, t)
        return [(op_name(L, t), tuple(t.contents.ne), tuple(t.contents.op_params)) for t in FC.graph_nodes(g)]


# ------------------------------------------------------------------ builders the wrapper does not declare

def view_tensor(b, a):
    return FC._bind(b.L, "ggml_view_tensor", [ctypes.c_void_p, G.T])(b.c, a)


def as_inplace(b, a, node):
    """`node` (an op on `a`) recast as the node its _inplace builder makes: a view of `a` with the op, the
    parameters and the sources of `node`."""
    r = view_tensor(b, a)
    r.contents.op = node.contents.op
    for k in range(16):
        r.contents.op_params[k] = node.contents.op_params[k]
    for k in range(10):
        r.contents.src[k] = node.contents.src[k]
    return r


def inplace(b, name, argtypes, a, *args):
    """ggml_<name>_inplace(ctx, a, *args) where the library exports it; else the same node built by hand."""
    fn = FC._bind(b.L, f"ggml_{name}_inplace", [ctypes.c_void_p, G.T] + list(argtypes))
    if fn:
        return fn(b.c, a, *args)
    return as_inplace(b, a, getattr(b.L, f"ggml_{name}")(b.c, a, *args))


def op_code(L, name):
    return next(i for i in range(76) if L.ggml_op_name(i).decode() == name)


def diag_mask(b, a, n_past, zero):
    return FC.diag_mask_zero(b.L, b.c, a, n_past) if zero else b.L.ggml_diag_mask_inf(b.c, a, n_past)


# ================================================================== A. forced fallbacks
#
# cpu_order.h: S = parallel double sum, A = sum |term|, B = 4 n A 2^-53; lo = (float)((S - B) / n) and
# hi = (float)((S + B) / n); lo != hi -> one lane replays the CPU's chain.

def pow2_terms(v):
    """The powers of two that add up to the dyadic v > 0, largest first."""
    m, e = math.frexp(v)
    m, e = int(math.ldexp(m, 53)), e - 53
    return [p2(e + i) for i in range(53, -1, -1) if (m >> i) & 1]


def squares_of(v):
    """Powers of two whose squares add up to v: an odd power of two takes two equal terms."""
    out = []
    for p in pow2_terms(v):
        e = math.frexp(p)[1] - 1
        out += [p2(e // 2)] if e % 2 == 0 else [p2((e - 1) // 2)] * 2
    return out


def group_start(n, m, where, lo, even=False):
    """First index of a row's m big terms: at the front (from lo), in the middle (crossing n / 2: another j
    slice, another 256-element block) or at the end (rows of 128 and more keep 48 - m elements of dust behind
    them, so that a case's columns of different k share their starts)."""
    s = {"front": lo, "mid": max(lo, min(n // 2 - 3, n - m)), "end": n - m if n < 128 else n - 48}[where]
    return s - s % 2 if even else s


def exact32(x):
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x), "row not representable in float"
    return x32


def sum_row(n, k=0, where="front", probe=None, lo=0):
    """A row whose sum / n is the midpoint above 1 + k 2^-20: the big terms n, n k 2^-20 and n 2^-24, every other
    element n 2^-54 (a quarter of the double sum's ulp once the big terms are in: the CPU's chain loses each
    one added after them and rounds the tie to even; added before them they lift the sum over the tie). With a
    probe, 1 + k 2^-20 of the first term moves to element `probe`: x - mean is 0 or -2^-23 there."""
    head = n - 1 if probe is not None else n
    big = [float(head)] + ([head * k * p2(-20)] if k else []) + [n * p2(-24)]
    x = np.full(n, n * p2(-54))
    s = group_start(n, len(big), where, lo)
    x[s:s + len(big)] = big
    if probe is not None:
        assert probe < s or probe >= s + len(big)
        x[probe] = 1.0 + k * p2(-20)
    return exact32(x), s


def sq_row(n, k=0, where="front", pm=False, lo=0, unit=-20):
    """A row whose sum of squares / n is the midpoint above 1 + k 2^unit, written as squares of powers of two;
    dust 2^-26 (square 2^-52). pm: every term as a +/- pair, so the mean is exactly zero in every summation order
    (which itself forces the mean's fallback: +-B / n round to different floats) and NORM's variance sees x^2."""
    half = 0.5 if pm else 1.0
    els = [e for part in (n * half, n * half * k * p2(unit), n * half * p2(-24)) if part for e in squares_of(part)]
    if pm:
        els = [s * e for e in els for s in (1.0, -1.0)]
    if len(els) > n:
        return None, 0
    x = np.full(n, p2(-26))
    if pm:
        x[1::2] = -p2(-26)
        if n % 2:
            x[-1] = 0.0
    s = group_start(n, len(els), where, lo, even=pm)
    if s < lo or s + len(els) > n - (n % 2 if pm else 0):
        return None, 0
    x[s:s + len(els)] = els
    return exact32(x), s


def seq_mean(terms):
    """The CPU's reduction: ggml_float sum, one term at a time; (float)(sum / n)."""
    return f32(np.cumsum(terms.astype(np.float64))[-1] / len(terms))


def certificate(terms, slack=1.0):
    """cpu_order.h's (lo, hi) for the exact sum S. The kernel's parallel S is within n 2^-53 A = B / 4 of it, so
    a straddle with slack 0.5 (B / 2 on either side) holds for whatever order the kernel adds in."""
    t = terms.astype(np.float64)
    n = len(t)
    S, A = math.fsum(t), math.fsum(np.abs(t))
    B = (4.0 * n * A * p2(-53) + 5e-324) * slack
    return f32((S - B) / n), f32((S + B) / n)


def norm_emul(x, rms, g=None, b=None, mean=None, msq=None, eps=EPS):
    """ggml_compute_forward_norm_f32 / _rms_norm_f32 (+ the MUL and ADD nodes) in numpy float32, with the
    reference's sequential double sums -- or with another float in place of a reduction's result."""
    x = x.astype(np.float32)
    v = x
    if not rms:
        v = x - (seq_mean(x) if mean is None else f32(mean))
    m = seq_mean(v * v) if msq is None else f32(msq)
    y = v * (f32(1.0) / np.sqrt(m + f32(eps)))
    if g is not None:
        y = y * g
    if b is not None:
        y = y + b
    return y


def reduction_terms(x, rms, red):
    """The float terms the reduction `red` ('mean', or 'msq': the variance / mean of squares) adds up."""
    x = x.astype(np.float32)
    if red == "mean":
        return x
    v = x if rms else x - seq_mean(x)
    return v * v


def other_candidates(x, rms, red):
    """The floats the certificate leaves open besides the CPU's result."""
    t = reduction_terms(x, rms, red)
    r = seq_mean(t)
    return [c for c in certificate(t) if c != r]


def scales_differ(x, rms):
    t = reduction_terms(x, rms, "msq")
    r = seq_mean(t)
    return all(f32(1.0) / np.sqrt(c + f32(EPS)) != f32(1.0) / np.sqrt(r + f32(EPS)) for c in certificate(t) if c != r)


def sq_row_pinned(n, where, pm, lo=0):
    """The first k of the family 1 + k 2^-23 whose two candidate means of squares give different scales
    1 / sqrtf(m + eps): they are one ulp apart, which sqrtf halves, so about every other k does (every float
    above 1 is in this family; the multiples of 2^-20 all round alike). k = 0 and unpinned if none fits the row."""
    for k in range(64):
        x, s = sq_row(n, k, where, pm, lo, unit=-23)
        if x is not None and scales_differ(x, not pm):
            return x, s, True
    x, s = sq_row(n, 0, where, pm, lo)
    assert x is not None
    return x, s, False


# ---- k_norm alone: tie rows and ordinary rows interleaved, one launch

def knorm_rows(n, rms):
    rows, forced = [], []

    def put(x, reds):
        forced.extend((len(rows), r, pin) for r, pin in reds)
        rows.append(x)

    def plain(seed):
        rows.append(u(seed, n, 3.0, 0.5))

    if rms:
        for i, where in enumerate(("front", "end", "mid")):
            x, _, pin = sq_row_pinned(n, where, False)
            put(x, [("msq", pin)])
            plain(20 + i)
    else:
        put(sum_row(n, 0, "front")[0], [("mean", True)])   # the issue's row: x[0] = n, x[1] = n 2^-24
        plain(10)
        put(sum_row(n, 3, "end")[0], [("mean", True)])
        x, _, pin = sq_row_pinned(n, "front", True)
        zero = n > 8   # the zero mean's other candidates are +-2^-49: they move the 2^-26 dust, which the 8-row has none of
        put(x, [("mean", zero), ("msq", pin)])
        plain(11)
        put(sum_row(n, 5, "mid")[0], [("mean", True)])
        x, _, pin = sq_row_pinned(n, "end", True)
        put(x, [("mean", zero), ("msq", pin)])
        plain(12)
        for k in range(6, 10):                                # the 1 + k 2^-20 family
            put(sum_row(n, k, ("front", "end")[k % 2])[0], [("mean", True)])
    return np.stack(rows), forced


def knorm_case(n, rms):
    X, forced = knorm_rows(n, rms)

    def fn(b):
        x = b.leaf(X, n, X.shape[0])
        return {"out": (b.L.ggml_rms_norm if rms else b.L.ggml_norm)(b.c, x, EPS)}

    add(f"forced/k_norm/{'rms' if rms else 'norm'}-n{n}", fn, launches=1, forced=forced, data={"X": X, "rms": rms, "kind": "k_norm"})


for _n in (8, 255, 256, 257, 768, ROW_LDS, ROW_LDS + 1):
    knorm_case(_n, False)
    knorm_case(_n, True)


# ---- the GEMV prologues: norm -> mul(g) [-> add(b)] -> mul_mat, one launch, mmv_order 1 (the CPU's bits)

PROBE = 5      # element of a mean column equal to one candidate mean; g[PROBE] = 2^24 makes x - mean visible
GROUP_LO = 8   # the first index a column's big terms may take
N_ROWS = 32    # rows of the weight matrix


class ForcedGemv:
    """Columns, g and b of one prologue case. kinds: per column (reduction, where). g is 2^-9 over every column's
    big terms (so that no activation dwarfs the rest), 2^-2 on each column's first big term (the largest
    activation of its block: a Q8_K block scale, an f32, then follows the norm's scale) and b is 0 there.
    For F16 activations the g on a variance / RMS column's first big term is tuned until the two candidate
    scales round that activation to different halves."""

    def __init__(self, wtype, K, rms, bias, kinds):
        self.wtype, self.K, self.rms, self.bias, self.kinds = wtype, K, rms, bias, kinds
        self.g = u(2, K, 0.5, 1.5)
        self.b = u(3, K, 1.0)
        cols, self.forced, starts = [], [], []
        for c, (red, where) in enumerate(kinds):
            if red == "mean":
                x, s = sum_row(K, (3 * c + K // 256) % 8, where, probe=PROBE, lo=GROUP_LO)
                self.forced.append((c, "mean", True))
                m = 3
            else:
                x, s, pin = sq_row_pinned(K, where, not rms, lo=GROUP_LO)
                if not rms:
                    self.forced.append((c, "mean", False))  # exactly zero: +-B / n changes no activation
                # Q8_0 activations keep an fp16 block scale and 8-bit levels: a scale one ulp off changes neither
                # (forced all the same: the replay must still cover every element); Q8_K's block scale is an f32
                self.forced.append((c, "msq", pin and wtype != Q8_0))
                m = int(np.sum(np.abs(x) > p2(-26)))
            cols.append(x)
            starts.append((s, m, red))
        self.X = np.stack(cols)
        for s, m, _ in starts:
            self.g[s:s + m] = p2(-9)
            self.b[s:s + m] = 0.0
        for s, _, _ in starts:
            self.g[s] = p2(-2)
        self.g[PROBE] = p2(24)
        if wtype == F16:
            for c, (s, _, red) in enumerate(starts):
                if red != "mean":
                    self.tune(c, s)

    def tune(self, c, s):
        x = self.X[c]
        t = reduction_terms(x, self.rms, "msq")
        r = seq_mean(t)
        others = [o for o in certificate(t) if o != r]
        v = x[s] if self.rms else x[s] - seq_mean(x)
        cand = (p2(-2) * (1.0 + np.arange(1 << 21) * p2(-23))).astype(np.float32)

        def act(m):
            return ((v * (f32(1.0) / np.sqrt(f32(m) + f32(EPS)))) * cand).astype(np.float16)

        flips = np.ones(len(cand), bool)
        for o in others:
            flips &= act(o) != act(r)
        if flips.any():
            self.g[s] = cand[np.argmax(flips)]

    def h(self, c, **override):
        """Column c of the MUL_MAT's src1 as the reference CPU computes it (or with a reduction overridden)."""
        return norm_emul(self.X[c], self.rms, self.g, self.b if self.bias else None, **override)

    def fn(self, b):
        L, c = b.L, b.c
        cols = len(self.kinds)
        x = b.leaf(self.X, self.K, cols)
        n = (L.ggml_rms_norm if self.rms else L.ggml_norm)(c, x, EPS)
        h = L.ggml_mul(c, n, b.leaf(self.g, self.K))
        if self.bias:
            h = L.ggml_add(c, h, b.leaf(self.b, self.K))
        w = b.leaf(FC.weight_bytes(L, self.wtype, self.K, N_ROWS, 6), self.K, N_ROWS, ttype=self.wtype)
        return {"out": L.ggml_mul_mat(c, w, h)}

    def fn_given_h(self, H):
        """mul_mat(W, H) alone, for the preconditions: H are activation columns computed in numpy."""
        def fn(b):
            w = b.leaf(FC.weight_bytes(b.L, self.wtype, self.K, N_ROWS, 6), self.K, N_ROWS, ttype=self.wtype)
            return {"out": b.L.ggml_mul_mat(b.c, w, b.leaf(H, self.K, H.shape[0]))}
        return fn


def gemv_case(path, wtype, K, rms, bias, kinds):
    d = ForcedGemv(wtype, K, rms, bias, kinds)
    what = "rms" if rms else "+".join(sorted({r for r, _ in kinds}, key=("mean", "msq").index)).replace("msq", "var")
    add(f"forced/{path}/{TYPE_NAME[wtype]}-K{K}-c{len(kinds)}-{what}-{'gb' if bias else 'g'}", d.fn, launches=1, orders=(1,),
        forced=d.forced, data={"gemv": d, "kind": path})


def gemv_family(path, wtype, Ks, cols):
    """Both modes; with b and without (g is what makes the chain a prologue); per K another placement first."""
    places = ("end", "mid", "front")
    for i, K in enumerate(Ks):
        w = places[i % 3:] + places[:i % 3]
        bias = i % 2 == 0
        if cols == 1:
            gemv_case(path, wtype, K, False, bias, [("mean", w[0])])
            gemv_case(path, wtype, K, False, not bias, [("msq", w[1])])
            gemv_case(path, wtype, K, True, bias, [("msq", w[0])])
        else:
            gemv_case(path, wtype, K, False, bias, [("mean", w[0]), ("msq", w[1]), ("mean", w[2])])
            gemv_case(path, wtype, K, True, not bias, [("msq", w[0]), ("msq", w[1]), ("msq", w[2])])


gemv_family("f16-registers", F16, (256, 520, 768), 3)     # stage_f16_activations, K <= 768: wave_mean_cpu_order<*, 12>
gemv_family("f16-registers", F16, (256, 768), 1)
gemv_family("f16-lds", F16, (776, 1024, 3072), 3)         # 768 < K: row_mean_cpu_order through LDS
gemv_family("f16-lds", F16, (3072,), 1)
gemv_family("q-prologue", Q4_K, (256, 512, 768), 3)       # norm_prologue: wave_mean_cpu_order<*, 12>, Q8_K activations
gemv_family("q-prologue", Q8_0, (256, 512, 768), 1)       # the same with Q8_0 activations
gemv_family("q-prologue1", Q4_K, (256, 512, 768), 1)      # norm_quant_prologue1: wave_mean_cpu_order4
gemv_family("q-prologue1", Q5_K, (512,), 1)

# reduction -> the case families that force it (DESIGN.md lists the ids a broken fallback fails)
REDUCTIONS = {
    "row_mean_cpu_order<false>": ("forced/k_norm/norm-", "forced/f16-lds/"),
    "row_mean_cpu_order<true>": ("forced/k_norm/rms-", "forced/f16-lds/"),
    "wave_mean_cpu_order<false>": ("forced/f16-registers/", "forced/q-prologue/"),
    "wave_mean_cpu_order<true>": ("forced/f16-registers/", "forced/q-prologue/"),
    "wave_mean_cpu_order4<false>": ("forced/q-prologue1/",),
    "wave_mean_cpu_order4<true>": ("forced/q-prologue1/",),
}


# ================================================================== B. RoPE

ROPE_T, ROPE_H, ROPE_CTX = 12, 2, 4096
# inside the table; its last row and one past it; far past it and negative
ROPE_POS = np.array([0, 1, 2, 37, 1000, 4094, ROPE_CTX - 1, ROPE_CTX, 5000, 100000, -1, -300], np.int32)
ROPE_TABLE = 4096  # rope_table_ensure: max(n_ctx, n_orig_ctx, 4096) positions


class Rope:
    def __init__(self, mode, D, n_dims, base=10000.0, fs=1.0, ext=0.0, af=1.0, n_orig=ROPE_CTX, beta_fast=32.0, beta_slow=1.0):
        self.mode, self.D, self.n_dims, self.base, self.fs, self.ext, self.af = mode, D, n_dims, base, fs, ext, af
        self.n_orig, self.beta_fast, self.beta_slow = n_orig, beta_fast, beta_slow

    def node(self, b, x, pos):
        return b.L.ggml_rope_custom(b.c, x, pos, self.n_dims, self.mode, ROPE_CTX, self.n_orig, self.base, self.fs, self.ext, self.af,
                                    self.beta_fast, self.beta_slow)

    def corr_dims(self):
        """ggml_rope_yarn_corr_dims in float32."""
        def dim(n_rot):
            return f32(self.n_dims) * np.log(f32(self.n_orig) / (f32(n_rot) * f32(2) * f32(np.pi))) / (f32(2) * np.log(f32(self.base)))
        return max(0.0, float(np.floor(dim(self.beta_fast)))), min(self.n_dims - 1.0, float(np.ceil(dim(self.beta_slow))))

    def mscale(self):
        """rope_yarn's magnitude as the reference computes it."""
        m = f32(self.af)
        if self.ext != 0.0:
            m = m * (f32(1.0) + f32(0.1) * np.log(f32(1.0) / f32(self.fs)))
        return float(m)

    def tag(self):
        return (f"m{self.mode}-D{self.D}-n{self.n_dims}-b{self.base:g}-s{self.fs:g}-e{self.ext:g}-a{self.af:g}")


def rope_x(D, seed=12):
    return u(seed, D * ROPE_H * ROPE_T, 1.0)


def rope_bound(r, x):
    """Outside the table cos and sin are rounded from double while the host's sincosf is within an ulp of them:
    1.5 ulp of a value <= 1, times mscale, times |x0| + |x1|, with headroom for the two roundings of the
    output: |d| <= 2^-21 mscale (|x0| + |x1|) per element; 0 where the row is only copied."""
    x = np.abs(x.reshape(ROPE_T, ROPE_H, r.D).astype(np.float64))
    pair = np.zeros_like(x)
    if r.mode == 0:
        s = x[..., 0::2] + x[..., 1::2]
        pair[..., 0::2] = s
        pair[..., 1::2] = s
    else:
        h = r.n_dims // 2
        s = x[..., :h] + x[..., h:2 * h]
        pair[..., :h] = s
        pair[..., h:2 * h] = s
    return p2(-21) * r.mscale() * pair


def rope_check(r, x):
    inside = (ROPE_POS >= 0) & (ROPE_POS < ROPE_TABLE)
    bound = rope_bound(r, x)

    def check(name, got, want):
        got, want = got.reshape(ROPE_T, ROPE_H, r.D), want.reshape(ROPE_T, ROPE_H, r.D)
        bad = []
        if not same_bits(got[inside], want[inside]):
            bad.append(f"{name}: {int(np.sum(got[inside] != want[inside]))} elements differ inside the table (identical bits expected)")
        d = np.abs(got[~inside].astype(np.float64) - want[~inside])
        ratio = float(np.max(d / np.maximum(bound[~inside], 1e-300) * (d > 0)))
        print(f"{name}: outside the table max |d| {float(d.max()):.3e}, {ratio:.3f} of the bound")
        if not np.all(d <= bound[~inside]):
            bad.append(f"{name}: outside the table {int(np.sum(d > bound[~inside]))} elements over the bound, worst {ratio:.2f} x")
        return bad
    return check


def rope_case(r, view=False):
    x = rope_x(r.D)

    def fn(b):
        if view:  # the first D of rows twice as wide; the rest holds NaN
            full = np.full((ROPE_T * ROPE_H, 2 * r.D), np.nan, np.float32)
            full[:, :r.D] = x.reshape(-1, r.D)
            X = b.leaf(full, 2 * r.D, ROPE_H, ROPE_T)
            xt = b.L.ggml_view_3d(b.c, X, r.D, ROPE_H, ROPE_T, X.contents.nb[1], X.contents.nb[2], 0)
        else:
            xt = b.leaf(x, r.D, ROPE_H, ROPE_T)
        return {"out": r.node(b, xt, b.leaf(ROPE_POS, ROPE_T, ttype=I32))}

    add(f"rope/{'view/' if view else ''}{r.tag()}", fn, check=rope_check(r, x), launches=1, data={"rope": [r]})


ROPE_SETS = []
for _mode in (0, 2):
    ROPE_SETS += [
        Rope(_mode, 128, 128),
        Rope(_mode, 128, 64, base=500000.0, fs=0.25, af=0.8),
        Rope(_mode, 64, 64, base=1e6, fs=0.25, ext=1.0),
        Rope(_mode, 80, 20, ext=1.0, af=0.8),
        Rope(_mode, 80, 80, base=500000.0, fs=0.25, ext=1.0, af=0.8),
        Rope(_mode, 128, 64, base=1e6, af=0.8),
        Rope(_mode, 64, 32, fs=0.25, ext=1.0),
        Rope(_mode, 80, 40, base=1e6, fs=0.25, af=0.8),
    ]
for _r in ROPE_SETS:
    rope_case(_r)
for _mode in (0, 2):
    rope_case(Rope(_mode, 80, 80, base=500000.0, fs=0.25, ext=1.0, af=0.8), view=True)
    rope_case(Rope(_mode, 64, 32), view=True)


def rope_multi(name, sets, repeat, replays):
    """Several ROPE nodes of different parameter sets over one x in one graph."""
    D = sets[0].D
    x = rope_x(D, 13)
    checks = {f"out{i}": rope_check(r, x) for i, r in enumerate(sets)}

    def fn(b):
        xt = b.leaf(x, D, ROPE_H, ROPE_T)
        pos = b.leaf(ROPE_POS, ROPE_T, ttype=I32)
        return {f"out{i}": r.node(b, xt, pos) for i, r in enumerate(sets)}

    add(name, fn, check=lambda n, g, w: checks[n](n, g, w), launches=len(sets), repeat=repeat, replays=replays, data={"rope": sets})


rope_multi("rope/two-nodes/m0-D64", [Rope(0, 64, 64, base=1e6, fs=0.25, ext=1.0), Rope(0, 64, 32, af=0.8)], 1, False)
rope_multi("rope/two-nodes/m2-D64", [Rope(2, 64, 64, base=1e6, fs=0.25, ext=1.0), Rope(2, 64, 32, af=0.8)], 1, False)
# four launches (the backend captures graphs of four and more), computed four times: direct, captured, replayed twice
rope_multi("rope/replayed/D80", [Rope(0, 80, 80, base=500000.0, fs=0.25, ext=1.0, af=0.8), Rope(2, 80, 20, ext=1.0, af=0.8),
                                 Rope(2, 80, 80, base=1e6), Rope(0, 80, 40, fs=0.25)], 4, True)


# ================================================================== C. layouts and edges

SHAPE = (16, 5, 3, 2)          # the leaf; permuted (0, 2, 1, 3) it is [16, 3, 5, 2] with nb[0] = 4
PERM = (16, 3, 5, 2)
BIN = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}


def n_of(ne):
    return int(np.prod(ne))


def permuted_a(b, ttype=F32, seed=30):
    a = b.leaf(u(seed, n_of(SHAPE), 2.0).astype(NP_TYPE[ttype]), *SHAPE, ttype=ttype)
    return b.L.ggml_permute(b.c, a, 0, 2, 1, 3)


def b_values(ne, seed=31):
    return u(seed, n_of(ne), 1.0, 1.75)   # in [0.75, 2.75]: a divisor too


def binary_case(opn, a_kind, b_ne, ta=F32, tb=F32, reference=True):
    """a: 'perm' (a [16, 5, 3, 2] leaf permuted to [16, 3, 5, 2]), 'cont', or 'inplace' (dst is a view of a)."""
    def values():
        a = u(30, n_of(SHAPE), 2.0).astype(NP_TYPE[ta])
        if a_kind == "perm":
            a = np.ascontiguousarray(a.reshape(SHAPE[::-1]).transpose(0, 2, 1, 3)).ravel()
        return a, b_values(b_ne).astype(NP_TYPE[tb])

    def fn(b):
        L = b.L
        if a_kind == "perm":
            a = permuted_a(b, ta)
        else:
            a = b.leaf(values()[0], *PERM, ttype=ta)
        bt = b.leaf(values()[1], *b_ne, ttype=tb)
        if opn == "sub" and tuple(b_ne) != PERM:
            # ggml_sub asserts same shapes (so does the reference's forward) while the backend's one kernel
            # broadcasts for all four ops: the node is an ADD node with SUB's op code
            node = L.ggml_add(b.c, a, bt)
            node.contents.op = op_code(L, "SUB")
            return {"out": as_inplace(b, a, node) if a_kind == "inplace" else node}
        if a_kind == "inplace":
            return {"out": inplace(b, opn, [G.T], a, bt)}
        return {"out": getattr(L, f"ggml_{opn}")(b.c, a, bt)}

    def expect():
        # one IEEE operation in float32 on the widened operands, rounded to the dst type (the type of a)
        a, bv = values()
        a = a.reshape(PERM[::-1]).astype(np.float32)
        bv = np.broadcast_to(bv.reshape(tuple(b_ne)[::-1] if len(b_ne) == 4 else (1, 1, 1, 1)).astype(np.float32), a.shape)
        return {"out": BIN[opn](a, bv).astype(NP_TYPE[ta]).ravel()}

    bn = "x".join(str(v) for v in b_ne)
    if opn == "sub" and tuple(b_ne) != PERM:
        reference = False
    add(f"layout/{opn}/{a_kind}-{TYPE_NAME[ta]}-b{bn}-{TYPE_NAME[tb]}", fn, expect=None if reference else expect,
        data={"expect": expect})


for _op in ("add", "sub", "mul", "div"):
    binary_case(_op, "perm", PERM)
    for _bne in ((1, 3, 5, 2), (16, 1, 5, 2), (16, 3, 1, 2), (16, 3, 5, 1), (1, 1, 1, 1), (1,)):
        binary_case(_op, "perm" if _bne[0] == 1 else "cont", _bne)
    binary_case(_op, "inplace", PERM)
    binary_case(_op, "inplace", (16, 1, 1, 1))
# the type pairs supports_op accepts. The reference CPU computes ADD of F16 + F32 and F16 + F16 (same shapes,
# ggml_compute_forward_add_f16_f32 / _f16_f16) and aborts on every other pair (ggml_compute_forward_add: F32 + F16;
# _sub / _mul / _div: anything but F32)
binary_case("add", "cont", PERM, F16, F32)
binary_case("add", "cont", PERM, F16, F16)
binary_case("add", "perm", PERM, F16, F32)
binary_case("add", "cont", PERM, F32, F16, reference=False)
binary_case("add", "perm", (16, 1, 5, 1), F16, F16, reference=False)   # F16 with a broadcast b: the reference asserts same shapes
binary_case("sub", "cont", PERM, F16, F32, reference=False)
binary_case("mul", "perm", PERM, F16, F16, reference=False)
binary_case("mul", "cont", (16, 1, 1, 1), F32, F16, reference=False)
binary_case("div", "cont", PERM, F16, F32, reference=False)
binary_case("div", "perm", (1,), F32, F16, reference=False)


def unary_case(opn, kind):
    """scale / gelu / silu of a source permuted (1, 0, 2, 3) -- nb[0] = 28 -- and in place. The reference's forwards
    assert contiguous operands (ggml_compute_forward_scale_f32, _gelu_f32, _silu_f32), so it gets cont(permute(x)):
    the same values, the same logical order."""
    ne = (7, 9, 3, 2)
    x = np.concatenate([u(32, n_of(ne) - 8, 6.0), np.array([-12.0, -10.0, 10.0, 12.0, 0.0, -0.0, 65504.0, 1e-8], np.float32)])

    def node(b, t):
        if opn == "scale":
            return inplace(b, "scale", [ctypes.c_float], t, 0.3) if kind == "inplace" else b.L.ggml_scale(b.c, t, 0.3)
        return inplace(b, opn, [], t) if kind == "inplace" else getattr(b.L, f"ggml_{opn}")(b.c, t)

    def fn(b):
        t = b.leaf(x, *ne)
        if kind == "perm":
            t = b.L.ggml_permute(b.c, t, 1, 0, 2, 3)
            if b.reference:
                t = b.L.ggml_cont(b.c, t)
        return {"out": node(b, t)}

    # on the reference the cont is a launch node of its own; on the backend only the op launches
    add(f"layout/{opn}/{kind}", fn, launches=1, same_graph=kind != "perm")


for _op in ("scale", "gelu", "silu"):
    unary_case(_op, "perm")
    unary_case(_op, "inplace")


def cpy_case(name, ts, td, src, dst):
    """src: 'perm' (permute 1, 2, 0, 3 of a [8, 6, 5, 2] leaf) or 'cont'; dst: 'cont' (same shape), 'perm' (a permuted
    view of a leaf) or 'reshaped' ([40, 12]: another shape, the same element count)."""
    ne = (8, 6, 5, 2)
    x = u(33, n_of(ne), 3.0).astype(NP_TYPE[ts])

    def fn(b):
        L, c = b.L, b.c
        s = b.leaf(x, *ne, ttype=ts)
        if src == "perm":
            s = L.ggml_permute(c, s, 1, 2, 0, 3)
        sne = tuple(s.contents.ne)
        if name == "cont":
            return {"out": L.ggml_cont(c, s)}
        if name == "dup":
            return {"out": FC._bind(L, "ggml_dup", [ctypes.c_void_p, G.T])(c, s)}
        if dst == "reshaped":
            d = new(L, c, td, 40, 12)
        elif dst == "perm":  # a leaf whose (2, 0, 1, 3) permutation has the source's shape
            d = new(L, c, td, sne[1], sne[2], sne[0], sne[3])
            b.feeds.append((d, np.zeros(n_of(ne), NP_TYPE[td])))
            d = L.ggml_permute(c, d, 1, 2, 0, 3)
            assert tuple(d.contents.ne) == sne
        else:
            d = new(L, c, td, *sne)
        return {"out": L.ggml_cpy(c, s, d)}

    add(f"layout/{name}/{TYPE_NAME[ts]}-{TYPE_NAME[td]}-src-{src}-dst-{dst}", fn)


for _ts, _td in ((F32, F16), (F16, F32), (F32, F32), (F16, F16)):
    cpy_case("cpy", _ts, _td, "perm", "cont")
    cpy_case("cpy", _ts, _td, "cont", "perm")
    cpy_case("cpy", _ts, _td, "perm", "reshaped")
for _ts in (F32, F16):
    cpy_case("cont", _ts, _ts, "perm", "cont")
    cpy_case("dup", _ts, _ts, "perm", "cont")


def cpy_q8_case(td, ne):
    """F32 -> Q8_0 / Q8_1 / Q8_K: the reference's from_float bytes (ggml_compute_forward_dup_f32 quantizes rows)."""
    x = u(34, n_of(ne), 4.0)
    x[:ne[0]] = 0.0           # a row of zero blocks: d = 0
    x[ne[0] + 3] = -9.0       # the largest magnitude negative
    x[2 * ne[0] + 40] = 9.0

    def fn(b):
        return {"out": b.L.ggml_cpy(b.c, b.leaf(x, *ne), new(b.L, b.c, td, *ne))}

    add(f"layout/cpy/f32-{TYPE_NAME[td]}-" + "x".join(str(v) for v in ne), fn, check=q8k_check if td == Q8_K else None)


def q8k_check(name, got, want):
    """block_q8_K is {float d; int8 qs[256]; int16 bsums[16]}. quantize_row_q8_K stores d = 0 and zero quants for
    an all-zero block and leaves its bsums as they were: those 32 bytes are whatever the buffer held, on either
    side, and are not compared. Every other byte is."""
    g, w = got.reshape(-1, 292), want.reshape(-1, 292)
    zero = np.ascontiguousarray(w[:, :4]).view(np.float32)[:, 0] == 0.0
    assert zero.any() and not zero.all()
    defined = np.ones(w.shape, bool)
    defined[zero, 260:] = False
    bad = int(np.sum((g != w) & defined))
    return [f"{name}: {bad} defined bytes differ (identical bytes expected)"] if bad else []


for _td in (Q8_0, Q8_1, Q8_K):
    cpy_q8_case(_td, (512, 5))
    cpy_q8_case(_td, (256, 3, 2))


def diag_mask_case(zero, ne, n_past, in_place):
    x = u(35, n_of(ne), 2.0)

    def fn(b):
        a = b.leaf(x, *ne)
        n = diag_mask(b, a, n_past, zero)
        return {"out": as_inplace(b, a, n) if in_place else n}

    add(f"layout/diag_mask_{'zero' if zero else 'inf'}/" + "x".join(str(v) for v in ne) + f"-past{n_past}{'-inplace' if in_place else ''}",
        fn, launches=1)


for _zero in (False, True):
    for _past in (0, 1, 10, 11, 40):       # ne0 = 11: 0, 1, ne0 - 1, ne0 and beyond
        diag_mask_case(_zero, (11, 7, 3), _past, False)
    diag_mask_case(_zero, (11, 7, 3), 1, True)
    diag_mask_case(_zero, (300, 9, 2), 295, True)   # more than one block


ROW_LENGTHS = (1, 2, 255, 256, 257, ROW_LDS, ROW_LDS + 1)


def norm_layout_case(rms, n, kind):
    """kind: 'cont' (3 rows), 'strided' (the first n of rows n + 3 wide, [n, 2, 2]: the rest holds NaN) or 'inplace'."""
    def fn(b):
        L, c = b.L, b.c
        if kind == "strided":
            full = np.full((4, n + 3), np.nan, np.float32)
            full[:, :n] = u(36, 4 * n, 3.0, 0.5).reshape(4, n)
            X = b.leaf(full, n + 3, 2, 2)
            x = L.ggml_view_3d(c, X, n, 2, 2, X.contents.nb[1], X.contents.nb[2], 0)
        else:
            x = b.leaf(u(36, 3 * n, 3.0, 0.5), n, 3)
        name = "rms_norm" if rms else "norm"
        if kind == "inplace":
            return {"out": inplace(b, name, [ctypes.c_float], x, EPS)}
        return {"out": getattr(L, f"ggml_{name}")(c, x, EPS)}

    add(f"layout/{'rms_norm' if rms else 'norm'}/n{n}-{kind}", fn, launches=1)


for _rms in (False, True):
    for _n in ROW_LENGTHS:
        norm_layout_case(_rms, _n, "cont")
    for _n in (257, ROW_LDS, ROW_LDS + 1):
        norm_layout_case(_rms, _n, "strided")
    norm_layout_case(_rms, ROW_LDS + 1, "inplace")
    norm_layout_case(_rms, 257, "inplace")


def soft_max_case(n, mask=None, scale=1.0, in_place=False, inf=False):
    """[n, 3, 2] rows. mask: F16 or F32, [n, 5] -- taller than the 3 rows, its first 3 rows broadcast over ne2 -- with
    -inf entries. inf: the rows themselves hold -inf (never a whole row: the reference asserts sum > 0)."""
    rows = 6
    x = u(37, rows * n, 4.0).reshape(rows, n)
    if inf and n > 1:
        x[:, 1::3] = -np.inf
        x[2, 1:] = -np.inf        # one finite element left
    m = u(38, 5 * n, 2.0).reshape(5, n)
    if n > 1:
        m[:, n // 2:] = np.where(np.arange(n - n // 2) % 2, -np.inf, m[:, n // 2:])
        m[1, 1:] = -np.inf

    def fn(b):
        L, c = b.L, b.c
        a = b.leaf(x, n, 3, 2)
        mt = b.leaf(m.astype(NP_TYPE[mask]), n, 5, ttype=mask) if mask is not None else None
        if mask is None and scale == 1.0:
            node = L.ggml_soft_max(c, a)
        else:
            node = L.ggml_soft_max_ext(c, a, mt, scale, 0.0)
        return {"out": as_inplace(b, a, node) if in_place else node}

    tag = f"n{n}" + (f"-mask-{TYPE_NAME[mask]}" if mask is not None else "") + (f"-scale{scale:g}" if scale != 1.0 else "")
    add(f"layout/soft_max/{tag}{'-inf' if inf else ''}{'-inplace' if in_place else ''}", fn, launches=1)


for _n in ROW_LENGTHS:
    soft_max_case(_n)
    soft_max_case(_n, mask=F16 if _n % 2 else F32, scale=0.125, inf=_n > 1)
for _n in (257, ROW_LDS + 1):
    soft_max_case(_n, mask=F32 if _n % 2 else F16, scale=0.3)
    soft_max_case(_n, inf=True)
soft_max_case(ROW_LDS + 1, in_place=True)
soft_max_case(ROW_LDS + 1, mask=F16, scale=0.125, in_place=True, inf=True)
soft_max_case(257, in_place=True)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
