"""Hand-made F16 weight matrices and activation columns, an exact evaluator and the table of cases that
tests/test_f16_cases.py proves on the CPU and tests/test_f16_cases_gpu.py runs over every F16 mul_mat
route. numpy only: no GPU, no ctypes.

The reference computes y[c, n] = sum_k w[n, k] * f16(h[c, k]) in f32, h the src1 column (optionally the
output of norm | rms_norm -> mul(g) -> add(b)), then the graph's ADD(bias), ADD(residual) or GELU nodes
and CPYs of row views. A product of two halves has at most 22 significant bits: exact in f32.

Two classes of cases:
  E (exact in any order): every term of an element is a multiple of 2^u (u: the smallest exponent of the
    lowest set bit among the row's weights plus the same of the column's rounded activations, a lower
    bound of every term's) and the certificate sum|w * f16(h)| (+ |bias| + |residual|) is below 2^24 units of
    2^u, u >= -126: every partial sum of every summation order, fused or not, is an exact normal f32 (or
    0), so every kernel in either order must return the bits of the exact result. Below that bound the
    sums are exact in float64 as well, which is how they are evaluated here.
  S (range ends): weights over all finite f16 bit patterns, activations over the f16 range with f32
    mantissas (rounded on the way), the real eps = 1e-5 norm chain. Not exact: reference order is held to
    the reference CPU's bits; tree-order and MFMA kernels per element to
        |y - exact| <= gamma * sum|w * x^|,   gamma = (K + 3) 2^-24 / (1 - (K + 3) 2^-24)
    (x^ the f16-rounded activation computed with the reference's f32 element operations; K - 1 additions in
    any order, each at most 2^-24 relative to a partial sum no larger than sum|terms| -- Higham's
    gamma_{K-1} -- plus one rounding each for the bias, the residual and the store of the value: K + 3
    covers them; derived, not measured).
"""
import functools

import numpy as np

F32, F16 = 0, 1
NORM, RMS_NORM = 1, 2


# ------------------------------------------------------------------ number formats

def rne16(x):
    """f32 -> f16 with round-to-nearest-even, subnormals kept, overflow to inf (numpy's conversion; the
    reference's GGML_FP32_TO_FP16 is F16C's vcvtps2ph in the same mode)."""
    return np.asarray(x, np.float32).astype(np.float16)


def rtz16(x):
    """f32 -> f16 truncating the magnitude (a wrong converter, for the mutants)."""
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    bits = h.view(np.uint16).copy()
    bits[over] -= 1  # the next half toward zero (sign-magnitude)
    return bits.view(np.float16)


def flush16(h):
    """f16 subnormals -> signed zero (a flushing route, for the mutants)."""
    h = np.asarray(h, np.float16)
    bits = h.view(np.uint16).copy()
    bits[(bits & 0x7C00) == 0] &= 0x8000
    return bits.view(np.float16)


def odd_exponent(p):
    """u with p = odd * 2^u for nonzero p (a large u for p == 0)."""
    p = np.asarray(p, np.float64)
    m, e = np.frexp(np.abs(p))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    u = e - 53 + np.round(np.log2(np.maximum(low, 1))).astype(np.int64)
    return np.where(p == 0, 10 ** 6, u)


def gamma(K):
    n = (K + 3) * 2.0 ** -24
    return n / (1 - n)


# ------------------------------------------------------------------ the reference's element operations

def norm_chain(x, norm):
    """norm | rms_norm -> mul(g) -> add(b) of the columns x [B, K] as the reference computes them
    (ggml_compute_forward_norm_f32 / rms_norm_f32: double sums, f32 mean, f32 element operations);
    div: the length the sums are divided by (K; the mutants pass the padded length)."""
    x = np.asarray(x, np.float32)
    K = norm.get("div", x.shape[1])
    eps = np.float32(norm["eps"])
    if norm["mode"] == NORM:
        mean = (x.astype(np.float64).sum(1) / K).astype(np.float32)
        v = x - mean[:, None]
        var = ((v * v).astype(np.float64).sum(1) / K).astype(np.float32)
    else:
        v = x
        var = ((x * x).astype(np.float64).sum(1) / K).astype(np.float32)
    scale = np.float32(1.0) / np.sqrt(var + eps)
    y = v * scale[:, None]
    assert y.dtype == np.float32
    if norm.get("g") is not None:
        y = y * norm["g"][None, :]
    if norm.get("b") is not None:
        y = y + norm["b"][None, :]
    return y


def gelu_f32(x):
    """ggml_gelu_f32 as the reference's build evaluates it: (0.5f x)(1 + tanhf((c1 x) fmaf(c2 x, x, 1)))."""
    x = np.asarray(x, np.float32)
    a = np.float32(0.044715) * x
    t = (a.astype(np.float64) * x.astype(np.float64) + 1.0).astype(np.float32)  # the fma: one rounding
    arg = (np.float32(0.79788456080286535587989211986876) * x) * t
    return (np.float32(0.5) * x) * (np.float32(1.0) + np.tanh(arg.astype(np.float64)).astype(np.float32))


def gelu_table(v):
    """ggml_vec_gelu_f32: 0 at and below -10, v at and above 10, else the f16 table entry of f16(v)."""
    v = np.asarray(v, np.float32)
    t = rne16(gelu_f32(rne16(v).astype(np.float32))).astype(np.float32)
    return np.where(v <= -10, np.float32(0), np.where(v >= 10, v, t)).astype(np.float32)


# ------------------------------------------------------------------ builders of the class-E kinds
# A kind is f(K, N, B) -> dict(w f16 [N, K], x f32 [B, K], + norm / bias / resid / gelu / copies).

def _ints(seed, shape, lo=1, hi=8):
    """Non-zero integers in [-hi, -lo] + [lo, hi]; along axis 0 neighbours differ at every position."""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, shape) * rng.choice([-1, 1], shape)
    for i in range(1, shape[0]):
        same = a[i] == a[i - 1]
        a[i][same] = -a[i][same]
    return a.astype(np.float64)


def _row_scale(N, lo=-6):
    return 2.0 ** (np.arange(N) % 10 + lo)


def _col_scale(B):
    return 2.0 ** (np.arange(B) % 5)


def k_int(K, N, B, lo=-6):
    w = _ints(11, (N, K)) * _row_scale(N, lo)[:, None]
    x = _ints(12, (B, K)) * _col_scale(B)[:, None]
    return dict(w=w, x=x)


def k_inf(K, N, B):
    """E-int with an infinite last weight in every third row: that row's output is the infinity times the sign of
    the last activation in any order (every other term is finite, no opposite infinity, no zero activation). A
    kernel that multiplies a weight chunk read again at its clamped address by the zero padding of the
    activations (inf * 0) returns NaN instead: what the zeroing of the chunks past the row's end is for."""
    d = k_int(K, N, B)
    d["w"][1::3, -1] = np.where(d["w"][1::3, -1] > 0, np.inf, -np.inf)
    return d


ONEHOT_AT = lambda K: sorted({k for k in (0, 7, 8, 127, 128, K - 9, K - 8, K - 1) if 0 <= k < K})


def k_onehot(K, N, B):
    """Columns e_k, weights whose f16 bits are unique in (n % 64, k % 256): the output is a gather of W."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    bits = (0x3C00 + (n % 64) * 256 + (k % 256)).astype(np.uint16)  # 1.0 .. 65504
    w = bits.view(np.float16).astype(np.float64) * np.where((n + k) % 3 == 0, -1.0, 1.0)
    at = ONEHOT_AT(K)
    x = np.zeros((B, K))
    for c in range(B):
        x[c, at[c % len(at)]] = 1.0
    return dict(w=w, x=x)


# f32 activations that no f16 holds, with their RNE roundings: ties to even both ways, the largest finite
# value, the underflow boundary, a negative value that rounds to -0
ROUND_BIG = [(2049.0, 2048.0), (2051.0, 2052.0), (2053.0, 2052.0), (2055.0, 2056.0), (-2051.0, -2052.0), (-2049.0, -2048.0),
             (2049.0 - 2.0 ** -12, 2048.0), (2051.0 + 2.0 ** -12, 2052.0)]
ROUND_MAX = (65519.0, 65504.0)
ROUND_TINY = [(2.0 ** -25, 0.0), (1.5 * 2.0 ** -25, 2.0 ** -24), (-(2.0 ** -26), -0.0), (3 * 2.0 ** -25, 2.0 ** -23),
              (-(2.0 ** -25) * (1 + 2.0 ** -20), -(2.0 ** -24)), (5 * 2.0 ** -25, 2.0 ** -23), (2.0 ** -24 + 2.0 ** -26, 2.0 ** -24),
              (-(2.0 ** -30), -0.0)]


def k_round(K, N, B):
    """Even columns: values near 2048 (x^ a multiple of 4) with 65519 at every 64th position; odd columns:
    values around the f16 underflow boundary (x^ a multiple of 2^-24). Weights +-2^e, e per row."""
    k = np.arange(K)
    x = np.empty((B, K))
    for c in range(B):
        tab = ROUND_BIG if c % 2 == 0 else ROUND_TINY
        x[c] = np.array([v for v, _ in tab])[(k + c // 2) % len(tab)]
        if c % 2 == 0:
            x[c, (k % 64) == (5 * c) % 64] = ROUND_MAX[0]
    sign = np.where(_ints(13, (N, K)) > 0, 1.0, -1.0)
    return dict(w=sign * _row_scale(N)[:, None], x=x)


def k_subw(K, N, B):
    """Subnormal f16 weights j 2^-24 (j = 1 .. 1023: every mantissa bit) against activations +-2^(10 + c % 3)."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    w = (1 + (n * 7 + k * 13) % 1023) * 2.0 ** -24 * np.where((n + k // 3) % 2 == 0, 1.0, -1.0)
    x = np.where(_ints(14, (B, K)) > 0, 1.0, -1.0) * 2.0 ** (10 + np.arange(B) % 3)[:, None]
    return dict(w=w, x=x)


def k_subx(K, N, B):
    """Normal weights (integers * 2^e) against f32 activations (j +- 1/8) 2^-24 (j = 1 .. 127), which round to
    the f16 subnormals j 2^-24 (half of them upward: truncation gives j - 1)."""
    c, k = np.arange(B)[:, None], np.arange(K)[None, :]
    j = 1 + (k * 5 + c * 11) % 127
    x = (j * 2.0 ** -24 + np.where(k % 2 == 0, 1.0, -1.0) * 2.0 ** -27) * np.where((k + c) % 3 == 0, -1.0, 1.0)
    return dict(w=_ints(15, (N, K)) * _row_scale(N)[:, None], x=x)


def k_zero(K, N, B):
    """Rows of +0 / -0 weights, rows (+a, -a, +a, -a), rows of -1; columns of zeros and columns (+b, +b, -b, -b):
    every output is an exact +0.0 (as the reference's: its sums start from +0)."""
    assert K % 4 == 0
    k = np.arange(K)
    w = np.empty((N, K))
    for n in range(N):
        kind = n % 4
        if kind == 0:
            w[n] = np.where(k % 2 == 0, 0.0, -0.0)
        elif kind == 1:
            w[n] = np.where(k % 2 == 0, 1.0, -1.0) * 2.0 ** (n % 7 - 3)
        elif kind == 2:
            w[n] = -1.0
        else:
            w[n] = np.where(k % 2 == 0, -1.0, 1.0) * (1 + k // 4 % 5)
    x = np.empty((B, K))
    for c in range(B):
        x[c] = 0.0 if c % 2 == 0 else np.where(k % 4 < 2, 1.0, -1.0) * (1 + (k // 4 + c) % 7) * 2.0 ** (c % 3)
    return dict(w=w, x=x)


def k_epi(epi, copies):
    def f(K, N, B):
        # GELU: rows scaled 2^-12 .. 2^-3, so that most sums lie within the table's range (-10, 10)
        d = k_int(K, N, B, lo=-12 if epi == "gelu" else -6)
        rs = _row_scale(N, -12 if epi == "gelu" else -6)
        d["bias"] = _ints(16, (N, 1), 1, 40)[:, 0] * rs
        if epi == "resid":
            d["resid"] = _ints(17, (B, N), 1, 100) * rs[None, :]
        d["gelu"] = epi == "gelu"
        if copies and N >= 3:
            a = N // 3
            d["copies"] = [(a, min(N, 2 * a)), (min(N, 2 * a), N)]  # the K and V rows of a c_attn output
        return d
    return f


NORM_SIGNS = np.array([1, -1, -1, 1, -1, 1, 1, -1])  # four of each in every aligned 8


def k_norm(mode, shift, gb, epi=None, copies=False):
    """Columns of {m + a, m - a} in equal counts (in every aligned 8), a = 1; NORM: m = 0 or a power of two
    per column (shift) and eps = 3: mean m, variance 1, scale 1/2. RMS_NORM: |m| = 2 (shift) or 0, eps = 11 or 3:
    mean square 5 or 1, scale 1/4 or 1/2. g, b small integers (gb: "gb", "g", ""): h = +-g / 2 + b and the like.
    epi / copies: the epilogue of k_epi behind it (GPT-2's ln -> c_attn + bias + K/V copies, ln -> c_fc + bias + GELU)."""
    def f(K, N, B):
        assert K % 8 == 0
        k = np.arange(K)
        x = np.empty((B, K))
        for c in range(B):
            if mode == NORM:
                m = [4.0, -2.0, 16.0, 0.0, -8.0, 1.0, 32.0, -0.5][c % 8] if shift else 0.0
            else:
                m = [2.0, -2.0][c % 2] if shift else 0.0
            x[c] = m + NORM_SIGNS[(k + 3 * (k // 8) + c) % 8]
        eps = 3.0 if mode == NORM or not shift else 11.0
        g = np.array([1.0, -1.0, 2.0, -2.0, 3.0])[(k * 3 + k // 5) % 5] if gb else None
        b = np.array([4.0, -4.0, 6.0, -6.0, 5.0, -5.0, 7.0])[(k + k // 7) % 7] if gb == "gb" else None
        d = dict(w=_ints(18, (N, K)), x=x, norm=dict(mode=mode, eps=eps, g=g, b=b))
        if epi:
            if epi == "gelu":  # most sums within the table's range
                d["w"] = d["w"] * 2.0 ** (np.arange(N) % 6 - 8)[:, None]
            rs = 2.0 ** (np.arange(N) % 6 - 8) if epi == "gelu" else np.ones(N)
            d["bias"] = _ints(16, (N, 1), 1, 40)[:, 0] * rs
            if epi == "resid":
                d["resid"] = _ints(17, (B, N), 1, 100)
            d["gelu"] = epi == "gelu"
            if copies and N >= 3:
                d["copies"] = [(N // 3, min(N, 2 * (N // 3))), (min(N, 2 * (N // 3)), N)]
        return d
    return f


# ------------------------------------------------------------------ class S

def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def k_range(norm):
    def f(K, N, B):
        rng = np.random.default_rng(21)
        bits = rng.integers(0, 0x7C00, (N, K)).astype(np.uint16) | (rng.integers(0, 2, (N, K)).astype(np.uint16) << 15)
        w = bits.view(np.float16).astype(np.float64)  # every finite f16, subnormals included
        if norm:
            # the real norm chain: eps = 1e-5, g around 1, b small, inputs of a few units (GPT-2's ln_1 -> c_attn)
            x = _f32(rng.standard_normal((B, K)) * 2.0 + 0.25)
            g = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32)
            b = (0.1 * rng.standard_normal(K)).astype(np.float32)
            return dict(w=w, x=x, norm=dict(mode=NORM if norm == "norm" else RMS_NORM, eps=1e-5, g=g, b=b))
        # f32 mantissas over the exponents 2^-26 .. 2^15 (rounded to f16 on the way: up to 65504, down to 0)
        x = _f32((1.0 + rng.random((B, K))) * 2.0 ** rng.integers(-26, 16, (B, K)) * rng.choice([-1.0, 1.0], (B, K)))
        x = np.where(np.abs(x) >= 65520.0, np.sign(x) * 65519.0, x)  # (65520 rounds to inf)
        d = dict(w=w, x=x)
        d["bias"] = _f32(rng.standard_normal(N) * 2.0 ** rng.integers(-10, 30, N))
        return d
    return f


def k_range_resid(K, N, B):
    """The range case with a residual next to the bias, of magnitudes at which (y + bias) + resid and
    (y + resid) + bias differ."""
    d = k_range(None)(K, N, B)
    rng = np.random.default_rng(22)
    d["resid"] = _f32(rng.standard_normal((B, N)) * 2.0 ** rng.integers(-10, 30, (B, N)))
    return d


# ------------------------------------------------------------------ the table

def _case(cid, cls, kind, f32_only=False, needs=1):
    return dict(id=cid, cls=cls, kind=kind, f32_only=f32_only, needs=needs)


CASES = [
    _case("E-int", "E", k_int),
    _case("E-onehot", "E", k_onehot),
    _case("E-inf", "E", k_inf),
    _case("E-round", "E", k_round, f32_only=True),
    _case("E-subw", "E", k_subw),
    _case("E-subx", "E", k_subx, f32_only=True),
    _case("E-zero", "E", k_zero, needs=4),
    _case("E-epi-bias", "E", k_epi("bias", False)),
    _case("E-epi-resid", "E", k_epi("resid", False)),
    _case("E-epi-gelu", "E", k_epi("gelu", False)),
    _case("E-epi-bias-copies", "E", k_epi("bias", True)),
    _case("E-epi-resid-copies", "E", k_epi("resid", True)),
    _case("E-epi-gelu-copies", "E", k_epi("gelu", True)),
    _case("E-norm-gb", "E", k_norm(NORM, False, "gb"), needs=8),
    _case("E-norm-shift-gb", "E", k_norm(NORM, True, "gb"), needs=8),
    _case("E-norm-shift-g", "E", k_norm(NORM, True, "g"), needs=8),
    _case("E-norm-shift", "E", k_norm(NORM, True, ""), needs=8),
    _case("E-rms-gb", "E", k_norm(RMS_NORM, False, "gb"), needs=8),
    _case("E-rms-shift-gb", "E", k_norm(RMS_NORM, True, "gb"), needs=8),
    _case("E-rms-shift-g", "E", k_norm(RMS_NORM, True, "g"), needs=8),
    _case("E-norm-epi-bias-copies", "E", k_norm(NORM, True, "gb", "bias", True), needs=8),
    _case("E-norm-epi-gelu", "E", k_norm(NORM, True, "gb", "gelu"), needs=8),
    _case("E-rms-epi-resid", "E", k_norm(RMS_NORM, True, "g", "resid"), needs=8),
    _case("S-range", "S", k_range(None), f32_only=True),
    _case("S-range-resid", "S", k_range_resid, f32_only=True),
    _case("S-range-norm", "S", k_range("norm"), f32_only=True, needs=8),
    _case("S-range-rms", "S", k_range("rms"), f32_only=True, needs=8),
]
BY_ID = {c["id"]: c for c in CASES}
E_IDS = [c["id"] for c in CASES if c["cls"] == "E"]
S_IDS = [c["id"] for c in CASES if c["cls"] == "S"]
PLAIN = [c["id"] for c in CASES if "norm" not in c["id"] and "rms" not in c["id"]]
NORMS = [c["id"] for c in CASES if "norm" in c["id"] or "rms" in c["id"]]


def fits(cid, K):
    """K a multiple of what the case's construction needs (pairs, quads or aligned 8s)."""
    return K % BY_ID[cid]["needs"] == 0


def evaluate(d, K, conv=rne16, wmap=None):
    """The exact evaluation of a built case; conv / wmap: the activation converter and a map of the f16
    weights (the mutants pass wrong ones). Fills xh (f16 [B, K]), dot (long double [B, N]), abs, unit and the
    expected f32 output y [B, N] (class E: exact; class S: the f32 nearest the exact value)."""
    w16 = np.asarray(d["w"], np.float64).astype(np.float16)
    assert np.array_equal(w16.astype(np.float64), d["w"]), "a weight is no f16"
    x32 = np.asarray(d["x"], np.float64).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), d["x"]), "an activation is no f32"
    h = norm_chain(x32, d["norm"]) if d.get("norm") else x32
    xh = conv(h)
    wv = w16 if wmap is None else wmap(w16)
    ld = np.longdouble
    wfin = np.where(np.isfinite(wv), wv, np.float16(0)).astype(np.float64)  # (E-inf: the certificate is the finite terms')
    ab = np.abs(wfin) @ np.abs(xh.astype(np.float64)).T
    unit = odd_exponent(wfin).min(1)[None, :] + odd_exponent(xh.astype(np.float64)).min(1)[:, None]
    if (ab.T / np.exp2(np.minimum(unit, 1000).astype(np.float64))).max() < 2.0 ** 50:
        dot = (xh.astype(np.float64) @ wfin.T).astype(ld)  # every partial sum is an exact float64
    else:
        dot = np.stack([(wfin.astype(ld) * xh[c].astype(ld)[None, :]).sum(1) for c in range(xh.shape[0])])
    for n, k in zip(*np.nonzero(~np.isfinite(wv))):  # an infinite weight: the infinity times the activation's sign
        assert np.all(xh[:, k] != 0)
        dot[:, n] = np.float64(wv[n, k]) * np.sign(xh[:, k].astype(np.float64))
    out = dict(w16=w16, x32=x32, xh=xh, dot=dot, abs=ab.T.copy(), unit=unit)
    total, units = dot, out["abs"].copy()
    bias = resid = None
    if d.get("bias") is not None:
        bias = np.asarray(d["bias"], np.float64).astype(np.float32)
        assert np.array_equal(bias.astype(np.float64), d["bias"])
        total = total + bias.astype(ld)[None, :]
        units += np.abs(bias.astype(np.float64))[None, :]
        unit = np.minimum(unit, odd_exponent(bias)[None, :])
    if d.get("resid") is not None:
        resid = np.asarray(d["resid"], np.float64).astype(np.float32)
        assert np.array_equal(resid.astype(np.float64), d["resid"])
        total = total + resid.astype(ld)
        units += np.abs(resid.astype(np.float64))
        unit = np.minimum(unit, odd_exponent(resid))
    y = total.astype(np.float32)
    y = np.where(y == 0, np.float32(0.0), y)  # an exact zero sum is +0
    if d.get("gelu"):
        y = gelu_table(y)
    out.update(bias=bias, resid=resid, total=total, cert_abs=units, cert_unit=unit, y=y)
    return out


@functools.lru_cache(maxsize=None)
def materialize(cid, K, N, B):
    """The case at a size: the built dict with its evaluation merged in. Read-only, shared by every test."""
    c = BY_ID[cid]
    assert fits(cid, K), (cid, K)
    d = c["kind"](K, N, B)
    d.update(evaluate(d, K))
    d.update(id=cid, cls=c["cls"], K=K, N=N, B=B)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def certificate_E(m):
    """Class E: sum|terms| (+ |bias| + |resid|) in units of 2^u, and u, per element [B, N]."""
    return m["cert_abs"] / np.exp2(np.minimum(m["cert_unit"], 1000).astype(np.float64)), m["cert_unit"]


def expected_bits(m):
    return np.ascontiguousarray(m["y"], np.float32).view(np.uint32)


def tile_rows(m, n, copies=None):
    """The materialized case with its rows repeated down to n rows (the tall matrices: row r is row r % N)."""
    idx = np.arange(n) % m["N"]
    t = dict(m)
    t["N"] = n
    t["w16"] = m["w16"][idx]
    for k in ("bias",):
        t[k] = None if m[k] is None else m[k][idx]
    for k in ("resid", "y", "total", "cert_abs", "cert_unit", "dot", "abs", "unit"):
        t[k] = None if m[k] is None else np.ascontiguousarray(m[k][:, idx])
    t["copies"] = copies
    return t


def tree_bound(m):
    """Class S, tree order and MFMA: gamma(K) * (sum|w x^| + |bias| + |resid|) per element [B, N]."""
    return gamma(m["K"]) * m["cert_abs"]


# ------------------------------------------------------------------ mutants: wrong kernels in numpy
# Each returns the [B, N] f32 output a kernel with that defect would give (class E: exact arithmetic on the
# wrong operands; the defect alone moves the bits).

def _finish(m, dot, swap=False):
    v = dot.astype(np.float32)
    steps = [m["bias"][None, :] if m["bias"] is not None else None, m["resid"]]
    for s in (steps[::-1] if swap else steps):
        if s is not None:
            v = (v + s).astype(np.float32)
    v = np.where(v == 0, np.float32(0.0), v)
    return gelu_table(v) if m.get("gelu") else v


def _dot(w, xh):
    ld = np.longdouble
    return np.stack([(w.astype(ld) * xh[c].astype(ld)[None, :]).sum(1) for c in range(xh.shape[0])])


def mutant_drop_last_chunk(m):
    w = m["w16"].copy()
    w[:, -8:] = 0
    return _finish(m, _dot(w, m["xh"]))


def mutant_chunk_shift(m):
    """Reads weight chunk j at j + 1 (the last at its clamped address)."""
    K = m["K"]
    idx = np.minimum(np.arange(K) + 8, K - 8 + np.arange(K) % 8)
    return _finish(m, _dot(m["w16"][:, idx], m["xh"]))


def mutant_bias_dropped_on_ragged_rows(m):
    N = m["N"]
    v = m["dot"].astype(np.float32)
    b = m["bias"].copy()
    b[N - N % 4:] = 0
    v = (v + b[None, :]).astype(np.float32)
    if m["resid"] is not None:
        v = (v + m["resid"]).astype(np.float32)
    return gelu_table(v) if m.get("gelu") else v


def mutant_bias_by_row_group(m):
    """bias[row & ~3] for every row."""
    v = m["dot"].astype(np.float32)
    b = m["bias"][np.arange(m["N"]) & ~3]
    v = (v + b[None, :]).astype(np.float32)
    if m["resid"] is not None:
        v = (v + m["resid"]).astype(np.float32)
    return gelu_table(v) if m.get("gelu") else v


def mutant_resid_before_bias(m):
    return _finish(m, m["dot"], swap=True)


def mutant_mean_over_padded_length(m, pad=128):
    K = m["K"]
    kp = (K + pad - 1) // pad * pad
    h = norm_chain(m["x32"], dict(m["norm"], div=kp))
    return _finish(m, _dot(m["w16"], rne16(h)))


def mutant_flush_subnormals(m):
    return _finish(m, _dot(flush16(m["w16"]), flush16(m["xh"])))


def mutant_round_toward_zero(m):
    h = norm_chain(m["x32"], m["norm"]) if m.get("norm") else m["x32"]
    return _finish(m, _dot(m["w16"], rtz16(h)))


# ------------------------------------------------------------------ E-parts: one decode token's attention block
# GPT-2's block (attention -> F16 c_proj + bias + residual -> LN -> F16 c_fc + bias + GELU) with an exact output:
# n_kv = 2^p cached keys whose K rows all equal the token's, so every soft_max weight is exp(0) / 2^p = 2^-p
# exactly, integer V rows, an integer c_proj and bias, and the residual chosen so that the block's output is
# the input column of an E-norm-style case at K = 64 H: the consumer's certificate is that case's.

@functools.lru_cache(maxsize=None)
def parts_case(H, n_kv, consumer, F):
    D, E = 64, 64 * H
    cons = materialize(consumer, E, F, 1) if consumer else None
    target = cons["x32"][0].astype(np.float64) if cons else materialize("E-norm-shift-gb", E, 8, 1)["x32"][0].astype(np.float64)
    q = _ints(31, (1, E))[0]
    k = _ints(32, (1, E))[0]
    v = _ints(33, (n_kv, E))            # row n_kv - 1 is the token's own V
    att = v.sum(0) / n_kv               # multiples of 1 / n_kv, |att| <= 8: f16 values
    assert np.array_equal(att.astype(np.float16).astype(np.float64), att)
    wp = _ints(34, (E, E))
    bp = _ints(35, (E, 1), 1, 40)[:, 0]
    proj = wp @ att
    resid = target - bp - proj
    units = (np.abs(wp) @ np.abs(att) + np.abs(bp) + np.abs(resid)) * n_kv  # in units of 1 / n_kv
    d = dict(H=H, D=D, E=E, n_kv=n_kv, n_past=n_kv - 1, consumer=cons, F=F, target=target.astype(np.float32),
             cur=np.concatenate([q, k, v[-1]]).astype(np.float32), mem_k=np.tile(k, n_kv).astype(np.float32),
             mem_v=v.ravel().astype(np.float32), wp=wp.astype(np.float16), bp=bp.astype(np.float32), resid=resid.astype(np.float32),
             att=att, proj_units=units)
    d["mem_k"][-E:] = 0  # the token's own rows are written by the graph's K / V copies
    d["mem_v"][-E:] = 0
    assert np.array_equal(d["resid"].astype(np.float64), resid)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def mutant_last_chunk_not_zeroed(m, step=128):
    """Lanes past the row's end multiply the row's last chunk, read again at the clamped address, by the zero
    padding of the activations instead of a zeroed chunk: 0 for finite weights, NaN for an infinite one."""
    y = _finish(m, m["dot"]).copy()
    if m["K"] % step:
        y[:, ~np.isfinite(m["w16"][:, -8:]).all(1)] = np.nan
    return y
