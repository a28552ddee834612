// quant_decode.h -- the bit layout of every quantized weight format, written once: block field
// offsets and the integer decode of dwords already in registers (levels as int8x4 dwords, scales,
// mins). Loads stay with the kernels: how a kernel brings a block's dwords into registers (scalar
// base + 32-bit offset, aligned dwords + v_alignbyte, LDS staging) is a performance decision, not
// layout. Users: the GEMVs (mmv.hip, mmv_fused_impl.h), the MFMA GEMMs (mmq_exact.hip), the plane
// repack (mmq_planes.hip, the offsets) and the GET_ROWS dequantizer (ops.hip).
//
// The reference dot products whose integers these decoders reproduce:
//   Q4_0 x Q8_0   ggml_vec_dot_q4_0_q8_0   src/ggml-quants.c:3469-3874
//   Q8_0 x Q8_0   ggml_vec_dot_q8_0_q8_0   src/ggml-quants.c:4819+
//   Q4_1 x Q8_1   ggml_vec_dot_q4_1_q8_1   src/ggml-quants.c:4006-4039 (AVX2)
//   Q5_0 x Q8_0   ggml_vec_dot_q5_0_q8_0   src/ggml-quants.c:4279-4301 (AVX2)
//   Q5_1 x Q8_1   ggml_vec_dot_q5_1_q8_1   src/ggml-quants.c:4623-4648 (AVX2)
//   Q2_K x Q8_K   ggml_vec_dot_q2_K_q8_K   src/ggml-quants.c:5105-5169
//   Q3_K x Q8_K   ggml_vec_dot_q3_K_q8_K   src/ggml-quants.c:6001-6103
//   Q4_K x Q8_K   ggml_vec_dot_q4_K_q8_K   src/ggml-quants.c:7007-7502
//   Q5_K x Q8_K   ggml_vec_dot_q5_K_q8_K   src/ggml-quants.c:7833-8378
//   Q6_K x Q8_K   ggml_vec_dot_q6_K_q8_K   src/ggml-quants.c:8730-9310
//   IQ4_NL x Q8_0 ggml_vec_dot_iq4_nl_q8_0 src/ggml-quants.c:11733-11815
//   IQ4_XS x Q8_K ggml_vec_dot_iq4_xs_q8_K src/ggml-quants.c:11873-11967
// (The IQ4 codebook lookup, mi_iq4nl_levels, lives with its table in mi355x_common.h.)
#pragma once

#include "mi355x_common.h"

// ---------------------------------------------------------------- bytes of a dword

// the low / high nibbles of the four bytes of q, one per byte
__device__ __forceinline__ uint32_t qd_nib_lo(uint32_t q) { return q & 0x0F0F0F0Fu; }
__device__ __forceinline__ uint32_t qd_nib_hi(uint32_t q) { return (q >> 4) & 0x0F0F0F0Fu; }

// bit `bit` of each byte of h as bit 4 of that byte: the fifth bit of a 4-bit level (Q5_K's qh)
__device__ __forceinline__ uint32_t qd_bit4(uint32_t h, int bit) { return ((h >> bit) & 0x01010101u) << 4; }

// four fifth bits (bits 0..3 of x) to bit 4 of four bytes (Q5_0 / Q5_1's qh): bit b of
// x * 0x00204081 lands at b, b + 7, b + 14, b + 21 -- sixteen distinct positions, no carries -- of
// which 0, 8, 16, 24 are kept
__device__ __forceinline__ uint32_t qd_spread4(uint32_t x) { return (((x & 0xFu) * 0x00204081u) & 0x01010101u) << 4; }

// bytes of v (each below 128, at least SUB) -> bytes of v - SUB as int8, no carries between the
// bytes: (v + 128 - SUB) never borrows, the xor takes the 128 back out mod 256
template <uint32_t SUB> __device__ __forceinline__ uint32_t qd_sub_bytes(uint32_t v) {
    return ((v | 0x80808080u) - SUB * 0x01010101u) ^ 0x80808080u;
}
// Q4_0's q - 8 of four nibbles in the MFMA GEMMs: the same integers as qd_sub_bytes<8>, written as
// the one add the GEMMs compile to
__device__ __forceinline__ uint32_t qd_q40_center(uint32_t nib) { return (nib + 0x78787878u) ^ 0x80808080u; }

// ---------------------------------------------------------------- 32-element blocks
//
// T is the weight's ggml_type: Q4_0 (18 B: fp16 d, qs[16]), Q8_0 (34 B: fp16 d, int8 qs[32]),
// Q4_1 (20 B: fp16 d, m, qs[16]), Q5_0 (22 B: fp16 d, qh[4], qs[16]), Q5_1 (24 B: fp16 d, m,
// qh[4], qs[16]); the facts below are its row of the table in mi355x_types.h. In the nibble
// formats element j < 16 is the low nibble of qs[j], element j >= 16 the high nibble of
// qs[j - 16]; bit j of the little-endian qh is the fifth bit of element j.
// Values: Q4_0 (q - 8) d, Q5_0 (q - 16) d, Q4_1 / Q5_1 q d + m. Q4_1 / Q5_1 dot with Q8_1
// activations, whose per-block s = fp16(d * sum(qs)) lies as fp16 bits in act.s32.
// IQ4_NL (18 B: fp16 d, qs[16]) has Q4_0's geometry; its nibbles index the codebook kvalues_iq4nl
// (LUT), value d kvalues[q], nothing subtracted.
template <int T> struct q32_fmt {
    static constexpr bool Q8 = T == MI_TYPE_Q8_0;
    static constexpr bool HAS_M = mi_type(T).has_m;    // fp16 m after d, Q8_1 activations
    static constexpr bool HAS_QH = mi_type(T).has_qh;  // fifth bits
    static constexpr int BS = mi_type(T).bytes;
    static constexpr int QH = HAS_M ? 4 : 2;          // offset of qh
    static constexpr int QS = (HAS_M ? 4 : 2) + (HAS_QH ? 4 : 0);  // offset of the quants
    static constexpr int SUB = mi_type(T).sub;  // subtracted from every level
    static constexpr bool LUT = mi_type(T).lut;  // the nibbles index the IQ4 codebook
};

// ---------------------------------------------------------------- Q4_K / Q5_K
//
// Q4_K (144 B): fp16 d | fp16 dmin | scales[12] | qs[128]; Q5_K (176 B): ... scales[12] | qh[32] |
// qs[128]. Byte qs[32j + b] holds element 64j + b in its low nibble and element 64j + 32 + b in its
// high nibble (sub-blocks 2j and 2j + 1); bit k of qh[b] is the fifth bit of element 32k + b.
template <bool Q5> struct kq_fmt {
    static constexpr int BS = mi_type(Q5 ? MI_TYPE_Q5_K : MI_TYPE_Q4_K).bytes;
    static constexpr int SC = 4;             // offset of the 12 scale bytes
    static constexpr int QH = 16;            // offset of qh (Q5_K)
    static constexpr int QS = Q5 ? 48 : 16;  // offset of qs
};

// the levels of sub-blocks 2j (lo) and 2j + 1 (hi) of a dword q of qs[32j ..] and the dword h of the
// same bytes of qh
template <bool Q5>
__device__ __forceinline__ void qd_kq_levels(uint32_t q, uint32_t h, int j, uint32_t & lo, uint32_t & hi) {
    if constexpr (Q5) {
        lo = qd_nib_lo(q) | qd_bit4(h, 2 * j);
        hi = qd_nib_hi(q) | qd_bit4(h, 2 * j + 1);
    } else {
        lo = qd_nib_lo(q);
        hi = qd_nib_hi(q);
    }
}

// The 6-bit scales and mins of the eight sub-blocks from the 12 scale bytes, taken as three
// little-endian dwords s0 s1 s2 (get_scale_min_k4, src/ggml-quants.c:1357-1365). Two forms, which
// yield the same integers:
//   qd_kq_scale_min              one sub-block j, the reference's own statement;
//   qd_kq_scales4 / qd_kq_mins4  four sub-blocks 4H .. 4H + 3 at once, one per byte of a dword.
// (The streaming GEMV's FmtKQ keeps a third, branch-free form for a lane-dependent j: folding it
// moved that kernel's compiled code. k_mmqx / k_mmqw keep bit-field extracts at per-thread fixed
// positions, which is how they address the fields, not another statement of the layout.
// k_planes_repack (mmq_planes.hip) keeps the reference's byte-pointer statement: on three dwords its
// Q5_K instance fell from 8 waves to 3.)
__device__ __forceinline__ void qd_kq_scale_min(int j, uint32_t s0, uint32_t s1, uint32_t s2, int & sc, int & m) {
    auto byte = [&](int i) -> int {
        const uint32_t w = i < 4 ? s0 : (i < 8 ? s1 : s2);
        return (int) ((w >> (8 * (i & 3))) & 0xFF);
    };
    if (j < 4) {
        sc = byte(j) & 63;
        m = byte(j + 4) & 63;
    } else {
        sc = (byte(j + 4) & 0xF) | ((byte(j - 4) >> 6) << 4);
        m = (byte(j + 4) >> 4) | ((byte(j) >> 6) << 4);
    }
}
template <int H> __device__ __forceinline__ uint32_t qd_kq_scales4(uint32_t s0, uint32_t s2) {
    if constexpr (H == 0) return s0 & 0x3F3F3F3Fu;
    else return qd_nib_lo(s2) | ((s0 >> 2) & 0x30303030u);
}
template <int H> __device__ __forceinline__ uint32_t qd_kq_mins4(uint32_t s1, uint32_t s2) {
    if constexpr (H == 0) return s1 & 0x3F3F3F3Fu;
    else return qd_nib_hi(s2) | ((s1 >> 2) & 0x30303030u);
}

// ---------------------------------------------------------------- Q6_K
//
// A 210-byte block is ql[128] | qh[64] | int8 scales[16] | fp16 d; element e of the superblock is
// d * scales[e / 16] * (q - 32) with q in 0..63. For the 128-half h, byte p (0..31):
//   ql[64h + p]      low nibble -> element 128h + p,      high nibble -> element 128h + 64 + p
//   ql[64h + 32 + p] low nibble -> element 128h + 32 + p, high nibble -> element 128h + 96 + p
//   qh[32h + p]      bits 2t, 2t+1 -> bits 4, 5 of element 128h + 32t + p
// Blocks are only 2-byte aligned (210 = 2 * 105; rows of an odd superblock count are 2 mod 4).
struct q6k_fmt {
    static constexpr int BS = mi_type(MI_TYPE_Q6_K).bytes;
    static constexpr int QL = 0, QH = 128, SC = 192, D = 208;
};

// the dwords la = ql[64h + p ..], lb = ql[64h + 32 + p ..], hh = qh[32h + p ..] to q - 32 as int8x4
// of the elements 128h + 32t + p .. p + 3 in q[t * ST] (t = 0..3)
template <int ST = 1>
__device__ __forceinline__ void qd_q6k_levels(uint32_t la, uint32_t lb, uint32_t hh, int * q) {
    q[0 * ST] = (int) qd_sub_bytes<32>(qd_nib_lo(la) | ((hh & 0x03030303u) << 4));
    q[1 * ST] = (int) qd_sub_bytes<32>(qd_nib_lo(lb) | (((hh >> 2) & 0x03030303u) << 4));
    q[2 * ST] = (int) qd_sub_bytes<32>(qd_nib_hi(la) | (((hh >> 4) & 0x03030303u) << 4));
    q[3 * ST] = (int) qd_sub_bytes<32>(qd_nib_hi(lb) | (((hh >> 6) & 0x03030303u) << 4));
}

// ---------------------------------------------------------------- Q2_K / Q3_K
//
// Q2_K (84 B): scales[16] | qs[64] | fp16 d | fp16 dmin, element d (sc & 0xF) q - dmin (sc >> 4)
// with q in 0..3. Q3_K (110 B): hmask[32] | qs[64] | scales[12] | fp16 d, element
// d (sc - 32) (q - (hbit ? 0 : 4)) with the 6-bit sc as qd_q3k_scale unpacks it. Both pack the quants
// alike: byte qs[32h + b] holds at bit 2t element 128h + 32t + b (h = 0..1, t = 0..3, b = 0..31);
// bit 4h + t of hmask[b] is that element's high bit. Q2_K blocks are 4-byte aligned, Q3_K blocks
// 2-byte aligned (rows of an odd superblock count are 2 mod 4).
template <int T> struct q23k_fmt {
    static constexpr bool Q3 = T == MI_TYPE_Q3_K;
    static constexpr int BS = mi_type(T).bytes;
    static constexpr int QS = Q3 ? 32 : 16;   // offset of qs
    static constexpr int SC = Q3 ? 96 : 0;    // offset of scales
    static constexpr int D = Q3 ? 108 : 80;   // offset of d (Q2_K: dmin follows)
};

// sub-block t's 2-bit quants of a dword of qs, one per byte
__device__ __forceinline__ uint32_t qd_q2(uint32_t qs, int t) { return (qs >> (2 * t)) & 0x03030303u; }

// sub-block t's levels of a dword of qs (and, Q3_K, of the hmask dword of the same bytes, high bit
// 4h + t) as int8x4: Q2_K q in 0..3; Q3_K (q | hbit << 2) - 4 = q - (hbit ? 0 : 4)
template <bool Q3>
__device__ __forceinline__ int qd_q23k_levels(uint32_t qs, uint32_t hm, int h, int t) {
    const uint32_t q = qd_q2(qs, t);
    if constexpr (!Q3) return (int) q;
    else return (int) qd_sub_bytes<4>(q | (((hm >> (4 * h + t)) & 0x01010101u) << 2));
}

// Q3_K: sub-block j's scale minus 32 -- low four bits in the nibbles of scales[0..7], upper two in
// scales[8 + j % 4] at bit 2 (j / 4) (the kmask1 / kmask2 unpack of the reference)
__device__ __forceinline__ int qd_q3k_scale(const uint8_t * scales, int j) {
    const int lo = (scales[j & 7] >> (4 * (j >> 3))) & 0xF;
    return (lo | (((scales[8 + (j & 3)] >> (2 * (j >> 2))) & 3) << 4)) - 32;
}
// the same integers for the four sub-blocks 4g .. 4g + 3 at once, as int8x4, from the 12 scale bytes
// as three little-endian dwords a0 a1 a2
__device__ __forceinline__ uint32_t qd_q3k_scales4(uint32_t a0, uint32_t a1, uint32_t a2, int g) {
    const uint32_t lo = (g & 1) ? a1 : a0;
    return qd_sub_bytes<32>(((g & 2) ? qd_nib_hi(lo) : qd_nib_lo(lo)) | (((a2 >> (2 * g)) & 0x03030303u) << 4));
}

// Q2_K: the scale | min bytes of the four sub-blocks 8h + 2t + u (t = 0..3: the 16-byte range u of
// the 128-half h), byte t, from the dwords s0 = scales[8h ..] and s1 = scales[8h + 4 ..]; qd_nib_lo
// of it are the four scales, qd_nib_hi the four mins
__device__ __forceinline__ uint32_t qd_q2k_range4(uint32_t s0, uint32_t s1, int u) {
    return __builtin_amdgcn_perm(s1, s0, u ? 0x07050301u : 0x06040200u);
}

// ---------------------------------------------------------------- IQ4_XS
//
// IQ4_XS (136 B): fp16 d | u16 scales_h | scales_l[4] | qs[128]; sub-block ib (32 elements, quants
// qs[16 ib ..], element j < 16 the low nibble of byte j, element 16 + j its high nibble) has the
// 6-bit scale ls = (nibble ib of scales_l) | (bits 2 ib .. of scales_h) << 4 and the value
// d (ls - 32) kvalues_iq4nl[q]. Blocks are whole dwords (136 = 4 * 34) of rows that start on one.
// sub-block ib's scale minus 32 from the dword of scales_l and scales_h
__device__ __forceinline__ int qd_iq4xs_scale(uint32_t sl, uint32_t sh, int ib) {
    return (int) (((sl >> (4 * ib)) & 0xF) | (((sh >> (2 * ib)) & 3) << 4)) - 32;
}
