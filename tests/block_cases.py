"""Hand-made Q4_0 / Q8_0 / Q4_K / Q5_K blocks, hand-made Q8_0 / Q8_K activation rows, an exact
evaluator and the table of cases that tests/test_block_cases.py proves on the CPU and
tests/test_block_cases_gpu.py runs over every kernel route. numpy only: no GPU, no ctypes.

Per block of a weight row n and an activation column b the reference computes
    Q4_K / Q5_K:  d_a * d_w * T - d_a * dmin_w * U,   T = sum_j sc_j sum_{k in j} q_k q8_k,  U = sum_j m_j S_j
    Q4_0:         d_a * d_w * T,                       T = sum_k (q_k - 8) q8_k
    Q8_0:         d_a * d_w * T,                       T = sum_k q_k q8_k
with S_j the sum of the 32 activation quants of sub-block j (bsums[2j] + bsums[2j + 1]).

Two classes of cases:
  E (exact in any order): every scale product is an odd integer times a power of two 2^u and the
    certificate sum|d_a d_w sc q q8| + sum|d_a dmin m q8| (T and U parts not netted) is below 2^24
    of the smallest such 2^u of the element, with 2^u >= 2^-100: every partial sum of every summation
    order is an exact normal f32, so every kernel in either order must return the integer result's bits.
  S (saturating): the ends of the integer ranges, where f32 cannot hold every integer. The
    certificate is the reach (REACH below), asserted. Tree-order and MFMA kernels are held per element
    to (n + 3) 2^-24 sum|terms|, n the blocks combined in f32.
A -128 activation byte is outside the reference's Q4_0 / Q8_0 domain (its AVX2 dot products negate
the activations with sign_epi8, which cannot negate -128): hand-made Q8_0 activation rows stay within
[-127, 127]; Q8_K rows use -128 (the K-quant dot products multiply the activations as they lie).
"""
import functools

import numpy as np

Q4_0, Q8_0, Q4_K, Q5_K, Q8_K = 2, 8, 12, 13, 15
NAMES = {Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4_K", Q5_K: "q5_K"}
BLCK = {Q4_0: 32, Q8_0: 32, Q4_K: 256, Q5_K: 256, Q8_K: 256}
BYTES = {Q4_0: 18, Q8_0: 34, Q4_K: 144, Q5_K: 176, Q8_K: 292}
ACT = {Q4_0: Q8_0, Q8_0: Q8_0, Q4_K: Q8_K, Q5_K: Q8_K}
QMAX = {Q4_0: 15, Q4_K: 15, Q5_K: 31}

# the reach the class-S cases must attain (asserted by test_block_cases.py)
REACH = {
    Q4_K: dict(T=63 * 15 * 256 * 128, U=8 * 63 * 4096),
    Q5_K: dict(T=63 * 31 * 256 * 128, U=8 * 63 * 4096, pair=63 * 32 * 31 * 128 * 2),
    Q4_0: dict(T=32 * 8 * 127),
    Q8_0: dict(T=32 * 128 * 127),
}
assert REACH[Q4_K]["T"] == 30965760 and REACH[Q5_K]["T"] == 63995904 and REACH[Q5_K]["pair"] == 15998976 < 2 ** 24
assert REACH[Q8_0]["T"] < 2 ** 22


# ------------------------------------------------------------------ fp16 scales

def f16_bits(x):
    """The fp16 bits of x, which must be an fp16 value (the sign of -0.0 is kept)."""
    h = np.float16(x)
    assert float(h) == float(x), x
    return int(h.view(np.uint16))


def f16_value(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def _u16(v):
    return np.array([v], "<u2").view(np.uint8)


# ------------------------------------------------------------------ builders from fields (one block)

def q4_0(d_bits, q):
    """q: the 32 stored nibbles 0..15 (value q - 8)."""
    q = np.asarray(q, np.int64)
    assert q.shape == (32,) and q.min() >= 0 and q.max() <= 15
    return np.concatenate([_u16(d_bits), (q[:16] | (q[16:] << 4)).astype(np.uint8)])


def q8_0(d_bits, q):
    """A Q8_0 weight block or activation block: 32 int8 quants."""
    q = np.asarray(q, np.int64)
    assert q.shape == (32,) and q.min() >= -128 and q.max() <= 127
    return np.concatenate([_u16(d_bits), q.astype(np.int8).view(np.uint8)])


def pack_scales(sc, m):
    """The 12 bytes of eight 6-bit scales and mins (get_scale_min_k4's layout: j >= 4 straddle bytes)."""
    sc, m = np.asarray(sc, np.int64), np.asarray(m, np.int64)
    assert sc.shape == m.shape == (8,) and min(sc.min(), m.min()) >= 0 and max(sc.max(), m.max()) <= 63
    s = np.empty(12, np.int64)
    s[0:4] = sc[:4] | ((sc[4:] >> 4) << 6)
    s[4:8] = m[:4] | ((m[4:] >> 4) << 6)
    s[8:12] = (sc[4:] & 15) | ((m[4:] & 15) << 4)
    return s.astype(np.uint8)


def _nibbles_k(q):
    """qs[128] of a K-quant: chunk c holds sub-block 2c in the low and 2c + 1 in the high nibbles."""
    q = q.reshape(4, 2, 32)
    return ((q[:, 0] & 15) | ((q[:, 1] & 15) << 4)).astype(np.uint8).ravel()


def q4_K(d_bits, dmin_bits, sc, m, q):
    q = np.asarray(q, np.int64)
    assert q.shape == (256,) and q.min() >= 0 and q.max() <= 15
    return np.concatenate([_u16(d_bits), _u16(dmin_bits), pack_scales(sc, m), _nibbles_k(q)])


def q5_K(d_bits, dmin_bits, sc, m, q):
    """q 0..31: the low nibbles in qs, bit 4 of sub-block j's element l in bit j of qh[l]."""
    q = np.asarray(q, np.int64)
    assert q.shape == (256,) and q.min() >= 0 and q.max() <= 31
    hi = (q >> 4).reshape(8, 32)
    qh = (hi << np.arange(8)[:, None]).sum(0).astype(np.uint8)
    return np.concatenate([_u16(d_bits), _u16(dmin_bits), pack_scales(sc, m), qh, _nibbles_k(q)])


def q8_K(d, q, bsums=None):
    """A Q8_K activation superblock: f32 d, 256 int8 quants, the sixteen int16 sums of 16 (consistent by default)."""
    q = np.asarray(q, np.int64)
    assert q.shape == (256,) and q.min() >= -128 and q.max() <= 127
    if bsums is None:
        bsums = q.reshape(16, 16).sum(1)
    return np.concatenate([np.array([d], "<f4").view(np.uint8), q.astype(np.int8).view(np.uint8),
                           np.asarray(bsums, "<i2").view(np.uint8)])


BUILD = {Q4_0: q4_0, Q8_0: q8_0, Q4_K: q4_K, Q5_K: q5_K, Q8_K: q8_K}


# ------------------------------------------------------------------ inverses (any leading shape)

def parse(t, buf):
    """Blocks of type t, uint8 [..., BYTES[t]] -> their fields as arrays [..., field shape]:
    d_bits (and d as float64; Q8_K: d alone), dmin_bits / dmin, sc, m, q, bsums."""
    buf = np.ascontiguousarray(buf, np.uint8)
    assert buf.shape[-1] == BYTES[t]
    lead = buf.shape[:-1]

    def u16(o):
        return buf[..., o].astype(np.uint16) | (buf[..., o + 1].astype(np.uint16) << 8)

    if t == Q8_K:
        return dict(d=np.ascontiguousarray(buf[..., 0:4]).view("<f4")[..., 0].astype(np.float64),
                    q=buf[..., 4:260].view(np.int8).astype(np.int64),
                    bsums=np.ascontiguousarray(buf[..., 260:292]).view("<i2").astype(np.int64))
    out = dict(d_bits=u16(0))
    out["d"] = f16_value(out["d_bits"])
    if t == Q8_0:
        out["q"] = buf[..., 2:34].view(np.int8).astype(np.int64)
        return out
    if t == Q4_0:
        qs = buf[..., 2:18].astype(np.int64)
        out["q"] = np.concatenate([qs & 15, qs >> 4], axis=-1)
        return out
    out["dmin_bits"] = u16(2)
    out["dmin"] = f16_value(out["dmin_bits"])
    s = buf[..., 4:16].astype(np.int64)
    out["sc"] = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 15) | ((s[..., 0:4] >> 6) << 4)], axis=-1)
    out["m"] = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], axis=-1)
    o = 16 if t == Q4_K else 48
    qs = buf[..., o:o + 128].astype(np.int64).reshape(lead + (4, 1, 32))
    q = np.concatenate([qs & 15, qs >> 4], axis=-2).reshape(lead + (256,))
    if t == Q5_K:
        qh = buf[..., 16:48].astype(np.int64)[..., None, :]
        q = q + 16 * ((qh >> np.arange(8)[:, None]) & 1).reshape(lead + (256,))
    out["q"] = q
    return out


def dequantize(t, buf):
    """The intended values d * sc * q - dmin * m (K-quants), d * (q - 8), d * q: float64 [..., block]."""
    f = parse(t, buf)
    if t == Q4_0:
        return f["d"][..., None] * (f["q"] - 8)
    if t in (Q8_0, Q8_K):
        return f["d"][..., None] * f["q"]
    return (f["d"][..., None] * np.repeat(f["sc"], 32, -1)) * f["q"] - f["dmin"][..., None] * np.repeat(f["m"], 32, -1)


# ------------------------------------------------------------------ the exact evaluator

def _odd_exponent(p):
    """u with p = odd * 2^u for nonzero float64 p (a large u for p == 0)."""
    m, e = np.frexp(np.abs(p))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    u = e - 53 + np.round(np.log2(np.maximum(low, 1))).astype(np.int64)
    return np.where(p == 0, 10 ** 6, u)


def evaluate(t, wq, xq, K):
    """Weight rows wq (uint8, N rows of type t) against activation rows xq (uint8, B rows of ACT[t]).
    Integer T, U per (column, row, block) in int64; the scaled sum in long double (64-bit mantissa: the
    products d_a d_w T are exact, their sum over the blocks is to 2^-63 relative). Returns a dict:
      y [B, N] long double; T, U [B, N, nb] int64; absT, absU [B, N] float64: the element's certificate sums
      sum|d_a d_w sc q q8| and sum|d_a dmin m q8|; unit [B, N]: u of the smallest 2^u among the element's
      nonzero scale products; pair [B, N, nb, 4] (K-quants): sc_2c T_2c + sc_2c+1 T_2c+1, the tree GEMV's pair term."""
    nb = K // BLCK[t]
    W = parse(t, np.asarray(wq, np.uint8).reshape(-1, nb, BYTES[t]))
    A = parse(ACT[t], np.asarray(xq, np.uint8).reshape(-1, nb, BYTES[ACT[t]]))
    da, aq = A["d"], A["q"]
    out = {}
    if t in (Q4_0, Q8_0):
        wv = W["q"] - 8 if t == Q4_0 else W["q"]
    else:
        wv = np.repeat(W["sc"], 32, -1) * W["q"]
    T = np.einsum("nsk,bsk->bns", wv, aq)
    absT = np.einsum("nsk,bsk->bns", np.abs(wv), np.abs(aq)).astype(np.float64)
    pd = da[:, None, :] * W["d"][None, :, :]  # exact in float64: 24 + 11 bits
    ld = np.longdouble
    y = (pd.astype(ld) * T.astype(ld)).sum(-1)
    out["absT"] = (np.abs(pd) * absT).sum(-1)
    unit = _odd_exponent(pd).min(-1)
    if t in (Q4_K, Q5_K):
        S = A["bsums"].reshape(A["bsums"].shape[:-1] + (8, 2)).sum(-1)
        U = np.einsum("nsj,bsj->bns", W["m"], S)
        absU = np.einsum("nsk,bsk->bns", np.repeat(W["m"], 32, -1), np.abs(aq)).astype(np.float64)
        pm = da[:, None, :] * W["dmin"][None, :, :]
        y = y - (pm.astype(ld) * U.astype(ld)).sum(-1)
        out["U"] = U
        out["absU"] = (np.abs(pm) * absU).sum(-1)
        unit = np.minimum(unit, _odd_exponent(pm).min(-1))
        Tj = np.einsum("nsjk,bsjk->bnsj", wv.reshape(wv.shape[:2] + (8, 32)), aq.reshape(aq.shape[:2] + (8, 32)))
        out["pair"] = Tj.reshape(Tj.shape[:3] + (4, 2)).sum(-1)
    else:
        out["U"] = np.zeros_like(T)
        out["absU"] = np.zeros_like(out["absT"])
    out.update(y=y, T=T, unit=unit)
    return out


def tree_bound(t, K, ev):
    """The per-element bound of the tree-order / MFMA kernels on class-S cases: (n + 3) 2^-24 sum|terms|,
    n the blocks combined in f32 -- one int -> f32 conversion, one product with the scales, one fma
    and an n-long chain, each at most half an ulp (2^-24 relative) of a partial sum no larger than sum|terms|."""
    n = K // BLCK[t]
    return (n + 3) * 2.0 ** -24 * (ev["absT"] + ev["absU"])


# ------------------------------------------------------------------ activation columns
# A column kind is f(t, K, c) -> (x, rows): x the F32 column (or None: hand-made only) and rows the
# Q8_0 / Q8_K bytes the reference's activation quantizer makes of x (test_block_cases.py proves it),
# or the hand-made row itself.

def _small(n, s):
    """Integers -3..3 with a period coprime to every block size, shifted per block s."""
    return ((np.arange(n) * 5 + 3 * s) % 7) - 3


def _act_rows(t, ints, e, flip):
    """ints [nb, QK] with exactly one +-127 per nonzero block; the quantizer's row for x = ints * 2^e.
    Q8_K: iscale = -127 / max: a positive maximum negates the quants and d (flip)."""
    a = ACT[t]
    blocks = []
    for s, q in enumerate(ints):
        if not q.any():
            blocks.append(np.zeros(BYTES[a], np.uint8))
        elif a == Q8_K:
            pos = q[np.argmax(np.abs(q))] > 0
            blocks.append(q8_K(-(2.0 ** e) if pos else 2.0 ** e, -q if pos else q))
        else:
            blocks.append(q8_0(f16_bits(2.0 ** e), q))
    return np.concatenate(blocks)


def _f32_col(kind, e):
    def f(t, K, c):
        qk = BLCK[ACT[t]]
        nb = K // qk
        ints = np.zeros((nb, qk), np.int64)
        for s in range(nb):
            q = _small(qk, s + c)
            if kind == "zeros" and s % 2 == 1:
                continue  # all-zero blocks between the others (d_a = 0)
            if kind == "subsign":
                # per sub-block of 32 alternating signs: S_j = -63 or +63 (S & 63 = 1 or 63, S >> 6 = -1 or 0)
                mag = 1 + np.arange(qk) % 32 % 3
                sign = np.where((np.arange(qk) // 32 + s) % 2 == 0, -1, 1)
                q = mag * sign
            p = (5 * s + 11 * c + 1) % qk
            if kind == "subsign":
                q[p] = 127 * int(np.sign(q[p]))  # keeps the sub-block's sign (either sign of maximum turns up)
            else:
                q[p] = 127 if kind == "pos127" else -127
            ints[s] = q
        x = (ints * 2.0 ** e).astype(np.float32).ravel()
        return x, _act_rows(t, ints, e, None)
    return f


def _q8_col(kind, e):
    """Hand-made rows no F32 input quantizes to: -128 bytes (Q8_K), scales of either sign, all-127 rows."""
    def f(t, K, c):
        a = ACT[t]
        qk = BLCK[a]
        nb = K // qk
        lo = -128 if a == Q8_K else -127
        blocks = []
        for s in range(nb):
            if kind == "small":  # small integers with one extreme byte of each sign per block
                q = _small(qk, s + c)
                q[(5 * s + c) % qk] = lo
                q[(5 * s + c + 13) % qk] = 127
            elif kind == "max":
                q = np.full(qk, 127)
            elif kind == "min":
                q = np.full(qk, lo)
            else:  # "alt": sub-blocks (Q8_0: blocks) of +127 and of the minimum in turn
                q = np.where((np.arange(qk) // 32 + (s if qk == 32 else 0)) % 2 == 0, 127, lo)
            if kind == "small":
                d = 2.0 ** e * (-1 if (s + c) % 3 == 2 else 1)
            else:  # one sign per column; Q8_0 "alt": twice the scale under the negative blocks, so that rows of one fill do not cancel
                d = 2.0 ** (e + (1 if kind == "alt" and qk == 32 and s % 2 else 0)) * (-1 if c % 2 else 1)
            blocks.append(q8_K(d, q) if a == Q8_K else q8_0(f16_bits(d), q))
        return None, np.concatenate(blocks)
    return f


def _const_col(v):
    """An F32 constant column: every quant -127 under iscale = -127 / v (Q8_K), sign(v) * 127 in Q8_0."""
    def f(t, K, c):
        qk = BLCK[ACT[t]]
        nb = K // qk
        x = np.full(K, v, np.float32)
        if ACT[t] == Q8_K:
            d = np.float32(1) / (np.float32(-127) / np.float32(v))
            row = np.concatenate([q8_K(d, np.full(256, -127))] * nb)
        else:
            d = np.float16(np.float32(abs(v)) / np.float32(127))
            row = np.concatenate([q8_0(int(d.view(np.uint16)), np.full(32, 127 if v > 0 else -127))] * nb)
        return x, row
    return f


ACTS_E_F32 = [_f32_col("neg127", 0), _f32_col("pos127", -3), _f32_col("zeros", 4), _f32_col("subsign", 0),
              _f32_col("subsign", -3), _f32_col("pos127", 4), _f32_col("neg127", -3), _f32_col("zeros", 0)]
ACTS_E_Q8 = [_q8_col("small", 0), _q8_col("small", -9), _q8_col("small", 5)]
ACTS_S_F32 = [_const_col(0.5), _const_col(-2.0)]
ACTS_S_Q8 = [_q8_col("max", 0), _q8_col("min", 0), _q8_col("alt", -2)]


# ------------------------------------------------------------------ weight rows
# A row kind is f(t, nb, r) -> uint8 [nb * BYTES[t]]; the block index s rotates the feature, so that
# rows of several blocks meet every position.

ONE = f16_bits(1.0)
SC_MIXED = [1, 33, 62, 21, 17, 48, 35, 63]  # j >= 4: low nibble and high 2 bits both in use
M_MIXED = [63, 32, 16, 47, 31, 49, 15, 60]
PLANE_SC = {Q4_K: [1, 7, 8, 56, 63], Q5_K: [1, 3, 4, 12, 16, 48, 63]}  # one and all bits of each plane field


def _kq_row(fn):
    """K-quant row from fn(t, s, r) -> (d_bits, dmin_bits, sc[8], m[8], q[256])."""
    return lambda t, nb, r: np.concatenate([BUILD[t](*fn(t, s, r)) for s in range(nb)])


def _q0_row(fn):
    """Q4_0 / Q8_0 row from fn(t, s, r) -> (d_bits, q[32])."""
    return lambda t, nb, r: np.concatenate([BUILD[t](*fn(t, s, r)) for s in range(nb)])


def _one_hot(j, v=63):
    a = np.zeros(8, np.int64)
    a[j % 8] = v
    return a


def _qpat(t, s):
    return (np.arange(256) + s) % (QMAX[t] + 1)  # q_k = k mod 16 / k mod 32, shifted per block


def rows_scales(t):
    """Sub-block scale / min unpacking: sc_j = 63 alone, m_j = 63 alone with d = 0, mixed 6-bit values."""
    kinds = []
    for j in range(8):
        kinds.append(_kq_row(lambda t, s, r, j=j: (ONE, ONE, _one_hot(j + s), np.zeros(8, np.int64), _qpat(t, s))))
        kinds.append(_kq_row(lambda t, s, r, j=j: (0, ONE, np.full(8, 63), _one_hot(j + s), _qpat(t, s))))
    kinds.append(_kq_row(lambda t, s, r: (ONE, ONE, np.roll(SC_MIXED, s), np.roll(M_MIXED, s + 3), _qpat(t, s))))
    kinds.append(_kq_row(lambda t, s, r: (ONE, f16_bits(-1.0), np.roll(M_MIXED, s), np.roll(SC_MIXED, s + 5), _qpat(t, s))))
    return kinds


def rows_planes(t):
    """Plane fields (every sc the same plane value, q at its maximum) and quant positions: nibble fills
    0x0F / 0xF0, q = k mod 16 / 32, Q5_K qh fills 0x00, 0xFF, 0x55, 0xAA and one bit per j."""
    qm = QMAX[t]
    kinds = []
    for v in PLANE_SC[t]:
        kinds.append(_kq_row(lambda t, s, r, v=v: (ONE, 0, np.full(8, v), np.zeros(8, np.int64), np.full(256, qm))))

    def nib(lo, hi, qh):  # lo / hi: the nibble of even / odd sub-blocks; qh: the byte every qh[l] holds
        q = np.where(np.arange(256) // 32 % 2 == 0, lo, hi)
        return q + (16 * ((qh >> (np.arange(256) // 32)) & 1) if t == Q5_K else 0)

    for lo, hi in ((15, 0), (0, 15)):  # qs fills 0x0F, 0xF0
        for qh in ((0x00, 0xFF, 0x55, 0xAA) if t == Q5_K else (0,)):
            kinds.append(_kq_row(lambda t, s, r, lo=lo, hi=hi, qh=qh: (ONE, ONE, np.roll(SC_MIXED, s), np.full(8, 1), nib(lo, hi, qh))))
    if t == Q5_K:
        for j in range(8):
            kinds.append(_kq_row(lambda t, s, r, j=j: (ONE, 0, np.roll(SC_MIXED, s), np.zeros(8, np.int64), nib(0, 0, 1 << ((j + s) % 8)))))
    kinds.append(_kq_row(lambda t, s, r: (ONE, ONE, np.full(8, 63), np.full(8, 63), _qpat(t, s))))
    return kinds


def rows_block_scales(t):
    """Block scales: fp16 subnormals 2^-24 and 0x03FF, the minimum normal, 2^15, negative, -0.0 (the mins
    keep that row's result nonzero); small sc and q so that 1023 * T stays under 2^24."""
    small = lambda s: np.where(np.arange(256) % 2 == 0, (np.arange(256) // 2 * 3 + np.arange(256) // 32 + s) % 4, 0)
    ones = np.full(8, 1)
    kinds = []
    for d_bits, dmin_bits in ((0x0001, 0x0001), (0x03FF, 0x0001), (0x0001, 0x03FF), (0x0400, 0x0400), (0x7800, 0x7800),
                              (f16_bits(-1.0), f16_bits(-2.0)), (0x8000, ONE), (ONE, 0x8000), (0x8400, 0x0001)):
        kinds.append(_kq_row(lambda t, s, r, a=d_bits, b=dmin_bits: (a, b, ones, ones if b not in (0x03FF,) else _one_hot(s, 1), small(s + r))))
    return kinds


def rows_legacy(t):
    """Q4_0 / Q8_0 rows: the extreme bytes, every nibble position, and the block scales above."""
    if t == Q8_0:
        qs = [np.full(32, v) for v in (-128, -127, 127, 1, -1)]  # bytes 0x80, 0x81, 0x7F, 0x01, 0xFF
        qs.append(np.where(np.arange(32) % 2, -128, 127))
    else:
        qs = [np.full(32, 0), np.full(32, 15), np.arange(32) % 16, np.where(np.arange(32) < 16, 15, 0), np.where(np.arange(32) < 16, 0, 15)]
    kinds = []
    for i, q in enumerate(qs):
        kinds.append(_q0_row(lambda t, s, r, q=q: (ONE, np.roll(q, s))))
        kinds.append(_q0_row(lambda t, s, r, q=q: (f16_bits(-0.5) if s % 2 else f16_bits(4.0), np.roll(q, s))))  # negative d
    for d_bits in (0x0001, 0x03FF, 0x0400, 0x7800, 0x8001):
        # values +1 / -1 on every fourth position, 0 between: 1023 * T stays under 2^24 over 72 blocks
        sparse = np.where(np.arange(32) % 4 == 0, 1 - 2 * (np.arange(32) // 4 % 2), 0) + (8 if t == Q4_0 else 0)
        kinds.append(_q0_row(lambda t, s, r, a=d_bits, q=sparse: (a, np.roll(q, s))))
    kinds.append(_q0_row(lambda t, s, r: (0x8000 if s % 2 else ONE, np.roll(qs[2 if t == Q4_0 else 3], s))))  # -0.0 between 1.0 blocks
    return kinds


def rows_saturated(t):
    """Fills 0x00 (L) / 0xFF (H) under (d, dmin) in {(1, 1), (1, 0), (0, 1), (-1, 1)}, rows of H alone and
    of L / H pairs in each order (a one-block row is H: every output stays nonzero); sc and m on the even
    sub-blocks alone, against the sub-block-alternating activations. Q4_0: nibbles 0 / 15 under d = +-1;
    Q8_0: bytes 0x80 / 0x7F."""
    kinds = []
    if t in (Q4_K, Q5_K):
        def blk(t, d, dm, hi):
            v = 63 if hi else 0
            return (f16_bits(d), f16_bits(dm), np.full(8, v), np.full(8, v), np.full(256, QMAX[t] if hi else 0))
        for d, dm in ((1, 1), (1, 0), (0, 1), (-1, 1)):
            for pat in ("H", "LH", "HL"):
                kinds.append(lambda t, nb, r, d=d, dm=dm, pat=pat: np.concatenate(
                    [BUILD[t](*blk(t, d, dm, nb == 1 or pat[s % len(pat)] == "H")) for s in range(nb)]))
        even = np.where(np.arange(8) % 2 == 0, 63, 0)
        kinds.append(_kq_row(lambda t, s, r: (ONE, ONE, even, even[::-1].copy(), np.full(256, QMAX[t]))))
        kinds.append(_kq_row(lambda t, s, r: (f16_bits(-1.0), ONE, even[::-1].copy(), even[::-1].copy(), np.full(256, QMAX[t]))))
    else:
        lo, hi = (np.full(32, 0), np.full(32, 15)) if t == Q4_0 else (np.full(32, -128), np.full(32, 127))
        for d in (1, -1):
            for pat in ("H", "L", "LH", "HL"):
                kinds.append(_q0_row(lambda t, s, r, d=d, pat=pat: (f16_bits(d), hi if pat[s % len(pat)] == "H" else lo)))
        # (d = -1 with L on the even and H on the odd blocks meets the "alt" activations with every term positive)
    return kinds


# ------------------------------------------------------------------ the table

def _case(cid, t, cls, rows, acts):
    return dict(id=f"{NAMES[t]}-{cid}", type=t, cls=cls, rows=rows, acts=acts, f32=acts is ACTS_E_F32 or acts is ACTS_S_F32)


def _cases():
    out = []
    for t in (Q4_K, Q5_K):
        for name, rows in (("scales", rows_scales(t)), ("planes", rows_planes(t)), ("dscale", rows_block_scales(t))):
            out.append(_case(f"E-{name}-f32", t, "E", rows, ACTS_E_F32))
        out.append(_case("E-scales-q8", t, "E", rows_scales(t), ACTS_E_Q8))
        out.append(_case("E-dscale-q8", t, "E", rows_block_scales(t), ACTS_E_Q8))
        out.append(_case("S-fill-f32", t, "S", rows_saturated(t), ACTS_S_F32))
        out.append(_case("S-fill-q8", t, "S", rows_saturated(t), ACTS_S_Q8))
    for t in (Q4_0, Q8_0):
        out.append(_case("E-bytes-f32", t, "E", rows_legacy(t), ACTS_E_F32))
        out.append(_case("E-bytes-q8", t, "E", rows_legacy(t), ACTS_E_Q8))
        out.append(_case("S-fill-f32", t, "S", rows_saturated(t), ACTS_S_F32))
        out.append(_case("S-fill-q8", t, "S", rows_saturated(t), ACTS_S_Q8))
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}


def kind_of(i, n):
    """The kind of row (column) i among n kinds: the cycle shifts by one every round, so a kind's rows
    are n + 1 apart -- across 70 rows every kind meets different lanes and tile positions whatever n is."""
    return (i + i // n) % n


@functools.lru_cache(maxsize=None)
def materialize(cid, K, N, B):
    """The case at a size: (wq uint8 [N rows], x float32 [B * K] or None, xq uint8 [B rows], evaluation).
    Read-only, shared by every test that needs it."""
    c = BY_ID[cid]
    t = c["type"]
    nb = K // BLCK[t]
    wq = np.concatenate([c["rows"][kind_of(r, len(c["rows"]))](t, nb, r) for r in range(N)])
    cols = [c["acts"][kind_of(b, len(c["acts"]))](t, K, b) for b in range(B)]
    x = np.concatenate([col[0] for col in cols]) if c["f32"] else None
    xq = np.concatenate([col[1] for col in cols])
    ev = evaluate(t, wq, xq, K)
    for a in (wq, xq, x) + tuple(ev.values()):
        if a is not None:
            a.setflags(write=False)
    return wq, x, xq, ev


def certificate_E(ev):
    """Class E: (sum|T terms| + sum|U terms|) in units of the element's smallest scale product, and that unit's exponent."""
    return (ev["absT"] + ev["absU"]) / np.exp2(ev["unit"].astype(np.float64)), ev["unit"]


def expected_bits(ev):
    """The f32 bits of the exact result (class E: the result is an f32 by its certificate)."""
    y = ev["y"].astype(np.float32)
    return y.ravel().view(np.uint32)
