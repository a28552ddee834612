// mmv_fused_impl.h -- the streaming decode GEMV k_mmv_stream (see mmv_fused.hip for the design),
// its weight-format policies and launchers. Included by one translation unit per weight format
// (mmv_fused_q2k.hip, _q3k, _q4k, _q5k, _q6k, _q40, _q80, _q41, _q50, _q51, _iq4nl, _iq4xs) so that the kernel instances compile in parallel; each
// exports one mi_mmv_launch_* entry point that mmv_fused.hip's dispatcher calls.
#pragma once

#include <stdio.h>

#include <type_traits>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

// the norm prologue replays the CPU's rounding (cpu_order.h turns FMA contraction off); the rest
// of this file keeps the default contraction
#include "cpu_order.h"
#pragma clang fp contract(fast)

namespace {

// ------------------------------------------------------------------ activations in LDS
// layout per member: qs [NC][K] int8 | d [NC][K/QKA] f32 | s32 [NC][K/32] int16
// (s32: the integer sum of the block's 32 quants; Q8_1 activations -- formats with F::S1 -- keep the
// fp16 bits of the block's s = d * sum there instead)

struct lds_act {
    int8_t * qs;
    float * d;
    int16_t * s32;
};

template <int QKA>
__device__ __forceinline__ lds_act lds_carve(uint8_t * lds, int NC, int64_t K) {
    lds_act a;
    a.qs = (int8_t *) lds;
    a.d = (float *) (lds + NC * K);
    a.s32 = (int16_t *) (lds + NC * K + NC * (K / QKA) * 4);
    return a;
}

template <int QKA>
__host__ __device__ constexpr size_t lds_bytes(int NC, int64_t K) {
    return (size_t) NC * (K + (K / QKA) * 4 + (K / 32) * 2);
}

// reference-order scratch (per wave: rows x columns x F::ord_words), after the activations
__host__ __device__ constexpr size_t ord_offset(size_t act) { return (act + 15) & ~(size_t) 15; }

// whether format F takes Q8_1 activations (F::S1; absent: no)
template <class F, class = void> struct fmt_s1 : std::false_type {};
template <class F> struct fmt_s1<F, std::enable_if_t<F::S1>> : std::true_type {};

// one 256-element slice (four floats per lane) of column c into LDS
template <int QKA, bool S1 = false>
__device__ __forceinline__ void quantize_slice(float4 v4, int lane, const lds_act & a, int64_t K, int c, int sl) {
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    int8_t * qs = a.qs + c * K + sl * 256;
    if constexpr (QKA == 256) {
        // Q8_K (quantize_row_q8_K_reference as the reference's gcc -mfma build rounds it)
        uint32_t packed;
        int sum32;
        float dd;
        mi_q8K_superblock(v, lane, packed, sum32, dd);
        *(uint32_t *) (qs + lane * 4) = packed;
        if ((lane & 7) == 0) a.s32[c * (K / 32) + sl * 8 + (lane >> 3)] = (int16_t) sum32;
        if (lane == 0) a.d[c * (K / 256) + sl] = dd;
    } else {
        // Q8_0, AVX2 branch of quantize_row_q8_0 (src/ggml-quants.c:535-618): per 32-block
        // amax, d = amax/127 -> fp16 (RNE), id = 127/amax, q = round-half-even(x*id).
        // 8 lanes hold one block; max over the 8-lane group with DPP.
        float am = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
        uint32_t ab = __float_as_uint(am);
        ab = max(ab, (uint32_t) mi_dpp<MI_DPP_QP_1032>(0, (int) ab));
        ab = max(ab, (uint32_t) mi_dpp<MI_DPP_QP_2301>(0, (int) ab));
        ab = max(ab, (uint32_t) mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, (int) ab));
        const float amax = __uint_as_float(ab);
        const float id = amax != 0.0f ? 127.f / amax : 0.0f;
        uint32_t packed = 0;
        int s = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = (int) __builtin_rintf(__fmul_rn(v[i], id));
            s += q;
            packed |= ((uint32_t) (q & 0xFF)) << (8 * i);
        }
        s = mi_sum8(s);
        *(uint32_t *) (qs + lane * 4) = packed;
        if ((lane & 7) == 0) {
            const int blk = sl * 8 + (lane >> 3);
            a.d[c * (K / 32) + blk] = mi_h2f(mi_f2h(amax / 127.f));
            // Q8_1 (AVX2 quantize_row_q8_1, src/ggml-quants.c:806-867): s = fp16(d * (float) sum) with
            // the f32 d = amax / 127 before its own fp16 rounding
            if constexpr (S1) a.s32[c * (K / 32) + blk] = (int16_t) mi_mul_f2h(amax / 127.f, (float) s);
            else a.s32[c * (K / 32) + blk] = (int16_t) s;
        }
    }
}

// Q8_K of one superblock held by a 16-lane row, 16 consecutive elements per lane (a wave quantizes
// four superblocks at once): quantize_row_q8_K_reference (src/ggml-quants.c:3370-3407) as the
// reference's gcc -mfma build rounds it -- the first element of largest |x| keeps its sign
// (a row's max and min decide it; only when +a and -a both occur is the first index looked up),
// iscale = -127/max, q = min(127, RNE(iscale x)) by the fma bit trick, d = 1/iscale, zero
// superblocks d = 0. 16-lane DPP reductions (4 steps) instead of whole-wave ones with readlanes.
// `live`: this row's superblock exists (every lane takes part in the reductions).
__device__ __forceinline__ float mi_dppf_max16(float v) {
    auto f = [](int x) { return __int_as_float(x); };
    auto i = [](float x) { return __float_as_int(x); };
    v = fmaxf(v, f(mi_dpp<MI_DPP_QP_1032>(0, i(v))));
    v = fmaxf(v, f(mi_dpp<MI_DPP_QP_2301>(0, i(v))));
    v = fmaxf(v, f(mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, i(v))));
    v = fmaxf(v, f(mi_dpp<MI_DPP_ROW_MIRROR>(0, i(v))));
    return v;
}
__device__ __forceinline__ uint32_t mi_dpp_umin16(uint32_t v) {
    v = min(v, (uint32_t) mi_dpp<MI_DPP_QP_1032>(0, (int) v));
    v = min(v, (uint32_t) mi_dpp<MI_DPP_QP_2301>(0, (int) v));
    v = min(v, (uint32_t) mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, (int) v));
    v = min(v, (uint32_t) mi_dpp<MI_DPP_ROW_MIRROR>(0, (int) v));
    return v;
}
__device__ __forceinline__ void quantize_row16(const float4 (&v4)[4], int lane, const lds_act & a, int64_t K, int c, int sl, bool live) {
    float x[16];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        x[4 * u] = v4[u].x; x[4 * u + 1] = v4[u].y; x[4 * u + 2] = v4[u].z; x[4 * u + 3] = v4[u].w;
    }
    float mx = x[0], mn = x[0];
#pragma unroll
    for (int i = 1; i < 16; i++) {
        mx = fmaxf(mx, x[i]);
        mn = fminf(mn, x[i]);
    }
    mx = mi_dppf_max16(mx);
    mn = -mi_dppf_max16(-mn);
    float vmax = mx >= -mn ? mx : mn;
    const bool tie = mx == -mn && mx != 0.0f;
    if (__any(tie)) {  // +a and -a both largest in some row: the first one (key = 2 index + sign) wins
        uint32_t key = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 15; i >= 0; i--)
            if (fabsf(x[i]) == mx) key = (uint32_t) ((((lane & 15) * 16 + i) << 1) | (x[i] < 0.0f ? 1 : 0));
        key = mi_dpp_umin16(key);
        if (tie) vmax = (key & 1) ? mn : mx;
    }
    const float iscale = vmax != 0.0f ? -127.f / vmax : 0.0f;
    uint32_t w[4];
    int s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t pk = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float t = __builtin_fmaf(iscale, x[4 * j + e], 12582912.f);
            int q = (__float_as_int(t) & 0x007fffff) - 0x00400000;
            q = q < 127 ? q : 127;
            pk |= ((uint32_t) (q & 0xFF)) << (8 * e);
        }
        w[j] = pk;
        s = mi_dot4((int) pk, 0x01010101, s);
    }
    const int s32 = s + mi_dpp<MI_DPP_QP_1032>(0, s);  // lanes 2m, 2m + 1 of the row: elements 32 m ..
    if (live) {
        *(uint4 *) (a.qs + c * K + sl * 256 + (lane & 15) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        if ((lane & 1) == 0) a.s32[c * (K / 32) + sl * 8 + ((lane & 15) >> 1)] = (int16_t) s32;
        if ((lane & 15) == 0) a.d[c * (K / 256) + sl] = vmax != 0.0f ? 1.0f / iscale : 0.0f;
    }
}

// ------------------------------------------------------------------ weight formats

template <bool Q5>
struct FmtKQ {
    static constexpr bool KL = false;  // load() does not need K
    static constexpr int QKA = 256;  // activation block
    static constexpr int ITEM = 64;  // elements per item
    static constexpr int BS = mi_type(Q5 ? MI_TYPE_Q5_K : MI_TYPE_Q4_K).bytes;
    struct Regs {
        uint4 hdr, qa, qb;
        uint4 ha, hb;  // Q5 only
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        // row is wave-uniform and the lane offsets are 32-bit: scalar base + vector offset
        // addressing, no per-lane 64-bit address arithmetic per row
        const uint32_t s = (uint32_t) item >> 2, j = (uint32_t) item & 3;
        const uint32_t blk = s * BS;
        const uint32_t qp = blk + (Q5 ? 48 : 16) + 32 * j;
        r.hdr = *(const uint4 *) (row + blk);
        r.qa = *(const uint4 *) (row + qp);
        r.qb = *(const uint4 *) (row + qp + 16);
        if constexpr (Q5) {
            r.ha = *(const uint4 *) (row + blk + 16);
            r.hb = *(const uint4 *) (row + blk + 32);
        }
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        const int s = item >> 2, j = item & 3;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) s * 256 + 64 * j);
            const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
            const int alo[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const int ahi[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            const int ss = *(const int *) (a.s32 + c * (K / 32) + s * 8 + 2 * j);
            acc[c] = item_dot(r, j, alo, ahi, ss, a.d[c * (K / 256) + s], acc[c]);
        }
    }
    // one column's operands of an item, held in registers across rows (the item of a lane is the
    // same in every row)
    struct Act {
        int alo[8], ahi[8];
        int ss;
        float ad;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) {
        const int s = item >> 2, j = item & 3;
        const int4 * p = (const int4 *) (a.qs + (int64_t) s * 256 + 64 * j);
        const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
        const int l8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const int h8[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            v.alo[i] = l8[i];
            v.ahi[i] = h8[i];
        }
        v.ss = *(const int *) (a.s32 + s * 8 + 2 * j);
        v.ad = a.d[s];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int item, const Act & v, float acc) {
        return item_dot(r, item & 3, v.alo, v.ahi, v.ss, v.ad, acc);
    }
    // one item (superblock s, 64-group j) of one column, the column's quants / 32-sums / scale given
    __device__ static __forceinline__ float item_dot(const Regs & r, int j, const int (&alo)[8], const int (&ahi)[8], int ss, float ad, float acc) {
        const uint32_t q[8] = {r.qa.x, r.qa.y, r.qa.z, r.qa.w, r.qb.x, r.qb.y, r.qb.z, r.qb.w};
        uint32_t qlo[8], qhi[8];
        if constexpr (Q5) {
            const uint32_t h[8] = {r.ha.x, r.ha.y, r.ha.z, r.ha.w, r.hb.x, r.hb.y, r.hb.z, r.hb.w};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qlo[i] = (q[i] & 0x0F0F0F0Fu) | (((h[i] >> (2 * j)) & 0x01010101u) << 4);
                qhi[i] = ((q[i] >> 4) & 0x0F0F0F0Fu) | (((h[i] >> (2 * j + 1)) & 0x01010101u) << 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qlo[i] = q[i] & 0x0F0F0F0Fu;
                qhi[i] = (q[i] >> 4) & 0x0F0F0F0Fu;
            }
        }
        const float dw = mi_h2f((uint16_t) (r.hdr.x & 0xFFFF));
        const float dmw = mi_h2f((uint16_t) (r.hdr.x >> 16));
        // 6-bit scales / mins of sub-blocks 2j and 2j+1 (get_scale_min_k4,
        // src/ggml-quants.c:1357-1365) without divergent branches: j is lane-dependent
        const uint32_t sh = 16u * (uint32_t) (j & 1);
        const uint32_t x0 = r.hdr.y >> sh, x1 = r.hdr.z >> sh, x2 = r.hdr.w >> sh;
        int sc0, m0, sc1, m1;
        if (j < 2) {  // sub-blocks 0..3: plain 6-bit fields (a select, both sides are cheap)
            sc0 = (int) (x0 & 63);
            sc1 = (int) ((x0 >> 8) & 63);
            m0 = (int) (x1 & 63);
            m1 = (int) ((x1 >> 8) & 63);
        } else {      // sub-blocks 4..7: low 4 bits from bytes 8..11, high 2 bits from bytes 0..7
            sc0 = (int) ((x2 & 0xF) | (((x0 >> 6) & 3) << 4));
            sc1 = (int) (((x2 >> 8) & 0xF) | (((x0 >> 14) & 3) << 4));
            m0 = (int) (((x2 >> 4) & 0xF) | (((x1 >> 6) & 3) << 4));
            m1 = (int) (((x2 >> 12) & 0xF) | (((x1 >> 14) & 3) << 4));
        }
        int lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            lo = mi_dot4((int) qlo[i], alo[i], lo);
            hi = mi_dot4((int) qhi[i], ahi[i], hi);
        }
        // sc*lo + sc*hi and m*bsum + m*bsum in f32 are exact (|.| < 2^24: 63*32*31*127 and
        // 63*32*128 per term), i.e. (float) of the reference's int32 sums, without the
        // quarter-rate 32-bit integer multiplies
        const float sumi = fmaf((float) sc1, (float) hi, (float) sc0 * (float) lo);
        const float summ = fmaf((float) m1, (float) (ss >> 16), (float) m0 * (float) (int) (int16_t) (ss & 0xFFFF));
        // explicit fmas (the file contracts freely): the same bits in every kernel that inlines this
        return fmaf(ad, fmaf(-dmw, summ, dw * sumi), acc);
    }

    // CPU order (see ord_* below): per item (superblock s, 64-group j) the reference's eight int32
    // lanes l -- sc[2j] * (bytes 4l..4l+3 of the low nibbles . q8) + sc[2j+1] * (high nibbles) --
    // summed over the superblock's four items (a DPP quad: items 4s..4s+3 sit on adjacent lanes),
    // plus the mins lane m[2j] * bsum32[2j] + m[2j+1] * bsum32[2j+1]. Entry of superblock sb in the
    // scratch: [0..7] the eight int32 sums, [8..11] the four mins lanes (Q5_K: [8] their sum),
    // [12] d = y.d * x.d, [13] dmin = -(y.d * x.dmin).
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int) {
        const int s = item >> 2, j = item & 3;
        const uint32_t q[8] = {r.qa.x, r.qa.y, r.qa.z, r.qa.w, r.qb.x, r.qb.y, r.qb.z, r.qb.w};
        uint32_t qlo[8], qhi[8];
        if constexpr (Q5) {
            const uint32_t h[8] = {r.ha.x, r.ha.y, r.ha.z, r.ha.w, r.hb.x, r.hb.y, r.hb.z, r.hb.w};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qlo[i] = (q[i] & 0x0F0F0F0Fu) | (((h[i] >> (2 * j)) & 0x01010101u) << 4);
                qhi[i] = ((q[i] >> 4) & 0x0F0F0F0Fu) | (((h[i] >> (2 * j + 1)) & 0x01010101u) << 4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qlo[i] = q[i] & 0x0F0F0F0Fu;
                qhi[i] = (q[i] >> 4) & 0x0F0F0F0Fu;
            }
        }
        const float dw = mi_h2f((uint16_t) (r.hdr.x & 0xFFFF));
        const float dmw = mi_h2f((uint16_t) (r.hdr.x >> 16));
        const uint32_t sh = 16u * (uint32_t) (j & 1);
        const uint32_t x0 = r.hdr.y >> sh, x1 = r.hdr.z >> sh, x2 = r.hdr.w >> sh;
        int sc0, m0, sc1, m1;
        if (j < 2) {
            sc0 = (int) (x0 & 63);
            sc1 = (int) ((x0 >> 8) & 63);
            m0 = (int) (x1 & 63);
            m1 = (int) ((x1 >> 8) & 63);
        } else {
            sc0 = (int) ((x2 & 0xF) | (((x0 >> 6) & 3) << 4));
            sc1 = (int) (((x2 >> 8) & 0xF) | (((x0 >> 14) & 3) << 4));
            m0 = (int) (((x2 >> 4) & 0xF) | (((x1 >> 6) & 3) << 4));
            m1 = (int) (((x2 >> 12) & 0xF) | (((x1 >> 14) & 3) << 4));
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) s * 256 + 64 * j);
            const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
            const int alo[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const int ahi[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            int v[8];
#pragma unroll
            for (int l = 0; l < 8; l++) {
                // |products| < 2^23: the 24-bit multiplier is exact
                v[l] = __mul24(sc0, mi_dot4((int) qlo[l], alo[l], 0)) + __mul24(sc1, mi_dot4((int) qhi[l], ahi[l], 0));
                v[l] += mi_dpp<MI_DPP_QP_1032>(0, v[l]);
                v[l] += mi_dpp<MI_DPP_QP_2301>(0, v[l]);
            }
            const int ss = *(const int *) (a.s32 + c * (K / 32) + s * 8 + 2 * j);
            int pm = __mul24(m0, (int) (int16_t) (ss & 0xFFFF)) + __mul24(m1, ss >> 16);
            if constexpr (Q5) {
                pm += mi_dpp<MI_DPP_QP_1032>(0, pm);
                pm += mi_dpp<MI_DPP_QP_2301>(0, pm);
            }
            uint32_t * e = scr + c * cs + (slot >> 2) * 16;
            // lane j stores sums 2j and 2j+1 (all four lanes hold all eight after the quad sums),
            // as floats (exact: |sum| < 2^24), i.e. the reference's _mm256_cvtepi32_ps
            const int w0 = j == 0 ? v[0] : j == 1 ? v[2] : j == 2 ? v[4] : v[6];
            const int w1 = j == 0 ? v[1] : j == 1 ? v[3] : j == 2 ? v[5] : v[7];
            *(uint2 *) (e + 2 * j) = make_uint2(__float_as_uint((float) w0), __float_as_uint((float) w1));
            if (!Q5 || j == 0) e[8 + j] = __float_as_uint((float) pm);
            const float yd = a.d[c * (K / 256) + s];
            if (j == 2) e[12] = __float_as_uint(yd * dw);
            if (j == 3) e[13] = __float_as_uint(-(yd * dmw));
        }
    }
    // one chain step per superblock: acc[l] = fma(d, (float) sumi[l], acc[l]) (the reference's
    // _mm256_fmadd_ps) and the mins accumulator: Q4_K four lanes acc_m[k] = fma(dmin, prod[k],
    // acc_m[k]) (_mm_fmadd_ps), Q5_K one scalar summs += dmin * hsum(prod) (contracted by the
    // reference's -mfma build)
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int, float & A, float & M) {
        const float * e = (const float *) scr;
        const int nsb = n_items >> 2;
        const int lm = 8 + (Q5 ? 0 : (l & 3));
        for (int sb = 0; sb < nsb; sb++, e += 16) {
            A = fmaf(e[12], e[l], A);
            M = fmaf(e[13], e[lm], M);
        }
    }
    // scratch words per (row, column): one 16-word entry per superblock (+8: bank spread)
    static int ord_words(int nitems, int & stride) {
        stride = 0;
        return 16 * (nitems / 4) + 8;
    }
    __device__ static __forceinline__ float finish(float A, float M) {
        float z = A + __shfl_xor(A, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        if constexpr (Q5) return z + M;
        float m = M + __shfl_xor(M, 2, 8);
        m = m + __shfl_xor(m, 1, 8);
        return z + m;
    }
};

// Q4_0 (18 B) / Q8_0 (34 B) blocks: 2-byte aligned. Load the dwords covering the quants
// (aligned down) and re-align with v_alignbyte; d is a separate 2-byte load.
// LUT: IQ4_NL, Q4_0's block with the nibbles as indices into the codebook kvalues_iq4nl -- the same
// loads; the levels come from mi_iq4nl_levels (three v_perm_b32 per four), once per block and
// reused for every column, and nothing is subtracted. Its reference order keeps two accumulators.
template <bool Q8, bool LUT = false>
struct FmtQ0 {
    static_assert(!(Q8 && LUT), "the codebook indexes nibbles");
    static constexpr bool KL = false;
    static constexpr int QKA = 32;
    static constexpr int ITEM = 32;
    static constexpr int BS = mi_type(Q8 ? MI_TYPE_Q8_0 : MI_TYPE_Q4_0).bytes;
    static constexpr int NQ = Q8 ? 8 : 4;  // quant dwords per block
    struct Regs {
        uint32_t w[NQ + 1];  // the dwords covering d and the quants
        uint32_t off;        // byte offset of the block in w[0]: 0 or 2
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        // rows start 16-byte aligned (fused_mv_eligible), so the block's misalignment is a
        // function of the item alone; dword loads only (a 16-bit load of d gets a zero-extend
        // the compiler places right behind the load, which waits for it), on 32-bit lane offsets
        // from the wave-uniform row pointer
        const uint32_t blk = (uint32_t) item * BS;
        r.off = blk & 2;
        const uint32_t base = blk - r.off;
#pragma unroll
        for (int i = 0; i <= NQ; i++) r.w[i] = *(const uint32_t *) (row + base + 4 * i);  // 256 B tail slack
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        // d = bytes off..off+1 of w[0]; the quants start at byte off + 2
        uint32_t t[NL];
#pragma unroll
        for (int i = 0; i < NQ; i++) t[i] = r.off ? r.w[i + 1] : __builtin_amdgcn_alignbyte(r.w[i + 1], r.w[i], 2);
        const uint32_t dbits = (r.off ? r.w[0] >> 16 : r.w[0]) & 0xFFFF;
        const float dw = mi_h2f((uint16_t) dbits);
        if constexpr (LUT) levels(t);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 32);
            const int4 a0 = p[0], a1 = p[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            acc[c] = block_dot(t, dw, av, Q8 || LUT ? 0 : (int) a.s32[c * (K / 32) + item], a.d[c * (K / 32) + item], acc[c]);
        }
    }
    // LUT: the four quant dwords t[0..3] to the block's eight dwords of int8 levels, t[l] = elements
    // 4l..4l+3 (the reference's lane l)
    static constexpr int NL = LUT ? 8 : NQ;
    __device__ static __forceinline__ void levels(uint32_t (&t)[NL]) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int lo, hi;
            mi_iq4nl_levels8(t[i], lo, hi);
            t[i] = (uint32_t) lo;
            t[i + 4] = (uint32_t) hi;
        }
    }
    __device__ static __forceinline__ float block_dot(const uint32_t (&t)[NL], float dw, const int (&av)[8], int s32, float da, float acc) {
        int sumi = 0;
        if constexpr (Q8 || LUT) {
#pragma unroll
            for (int i = 0; i < 8; i++) sumi = mi_dot4((int) t[i], av[i], sumi);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                sumi = mi_dot4((int) (t[i] & 0x0F0F0F0Fu), av[i], sumi);
                sumi = mi_dot4((int) ((t[i] >> 4) & 0x0F0F0F0Fu), av[i + 4], sumi);
            }
            sumi -= 8 * s32;  // (q - 8) * y
        }
        return fmaf((float) sumi, dw * da, acc);
    }
    struct Act {
        int av[8];
        int s32;
        float da;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) {
        const int4 * p = (const int4 *) (a.qs + (int64_t) item * 32);
        const int4 a0 = p[0], a1 = p[1];
        const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int i = 0; i < 8; i++) v.av[i] = av[i];
        v.s32 = Q8 || LUT ? 0 : (int) a.s32[item];
        v.da = a.d[item];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int, const Act & v, float acc) {
        uint32_t t[NL];
#pragma unroll
        for (int i = 0; i < NQ; i++) t[i] = r.off ? r.w[i + 1] : __builtin_amdgcn_alignbyte(r.w[i + 1], r.w[i], 2);
        const uint32_t dbits = (r.off ? r.w[0] >> 16 : r.w[0]) & 0xFFFF;
        if constexpr (LUT) levels(t);
        return block_dot(t, mi_h2f((uint16_t) dbits), v.av, v.s32, v.da, acc);
    }

    // CPU order: the reference's eight int32 lanes l of mul_sum_i8_pairs_float -- elements 4l..4l+3
    // (Q4_0: low nibbles for l < 4, high nibbles of bytes 4(l-4).. for l >= 4, minus 8) -- and
    // d = x.d * y.d, stored transposed: scratch [l][slot] (row stride 68 words), d at [8][slot].
    // IQ4_NL (ggml_vec_dot_iq4_nl_q8_0, AVX2): the same lanes of codebook levels, nothing subtracted;
    // the chain then runs the even blocks into accum1 (A) and the odd ones into accum2 (M), and the
    // lanes are added before hsum_float_8.
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int S) {
        uint32_t t[NL];
#pragma unroll
        for (int i = 0; i < NQ; i++) t[i] = r.off ? r.w[i + 1] : __builtin_amdgcn_alignbyte(r.w[i + 1], r.w[i], 2);
        const uint32_t dbits = (r.off ? r.w[0] >> 16 : r.w[0]) & 0xFFFF;
        const float dw = mi_h2f((uint16_t) dbits);
        if constexpr (LUT) levels(t);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 32);
            const int4 a0 = p[0], a1 = p[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            uint32_t * e = scr + c * cs + slot;
#pragma unroll
            for (int l = 0; l < 8; l++) {
                int q;
                if constexpr (Q8 || LUT) {
                    q = mi_dot4((int) t[l], av[l], 0);
                } else {
                    const uint32_t nib = l < 4 ? (t[l] & 0x0F0F0F0Fu) : ((t[l - 4] >> 4) & 0x0F0F0F0Fu);
                    q = mi_dot4((int) nib, av[l], mi_dot4((int) 0xF8F8F8F8u, av[l], 0));  // (q - 8) . y
                }
                e[l * S] = __float_as_uint((float) q);  // exact; _mm256_cvtepi32_ps
            }
            e[8 * S] = __float_as_uint(dw * a.d[c * (K / 32) + item]);
        }
    }
    // acc[l] = fma(d_i, (float) q[i][l], acc[l]) over the blocks in order (_mm256_fmadd_ps)
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int S, float & A, float & M) {
        (void) M;
        const float * q = (const float *) scr + l * S;
        const float * d = (const float *) scr + 8 * S;
        int i = 0;
        if constexpr (LUT) {
            // (every chunk of a row starts at an even block: the scratch slot's parity is the block's)
            for (; i + 4 <= n_items; i += 4) {
                const float4 qq = *(const float4 *) (q + i);
                const float4 dd = *(const float4 *) (d + i);
                A = fmaf(dd.x, qq.x, A);
                M = fmaf(dd.y, qq.y, M);
                A = fmaf(dd.z, qq.z, A);
                M = fmaf(dd.w, qq.w, M);
            }
            for (; i < n_items; i++) {
                if (i & 1) M = fmaf(d[i], q[i], M);
                else A = fmaf(d[i], q[i], A);
            }
            return;
        }
        for (; i + 4 <= n_items; i += 4) {
            const float4 qq = *(const float4 *) (q + i);
            const float4 dd = *(const float4 *) (d + i);
            A = fmaf(dd.x, qq.x, A);
            A = fmaf(dd.y, qq.y, A);
            A = fmaf(dd.z, qq.z, A);
            A = fmaf(dd.w, qq.w, A);
        }
        for (; i < n_items; i++) A = fmaf(d[i], q[i], A);
    }
    // scratch words per (row, column): 9 rows (8 lanes + d) of S >= nitems words; S = 4 (mod 32)
    // keeps the eight lanes' 16-byte chain reads on distinct banks
    static int ord_words(int nitems, int & stride) {
        int S = (nitems + 3) & ~3;
        while (S % 32 != 4) S += 4;
        stride = S;
        return 9 * S;
    }
    __device__ static __forceinline__ float finish(float A, float M) {
        if constexpr (LUT) A = A + M;  // _mm256_add_ps(accum1, accum2)
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A + __shfl_xor(A, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        return z + __shfl_xor(z, 1, 8);
    }
};
using FmtIQ4NL = FmtQ0<false, true>;

// Q4_1 (20 B: fp16 d, m, qs[16]), Q5_0 (22 B: fp16 d, qh[4], qs[16]) and Q5_1 (24 B:
// fp16 d, m, qh[4], qs[16]) blocks of 32. Element j < 16 is the low nibble of qs[j], element j >= 16
// the high nibble of qs[j - 16]; bit j of the little-endian qh is its fifth bit. Values q d + m
// (Q4_1 / Q5_1, against Q8_1 activations: S1) resp. (q - 16) d (Q5_0, against Q8_0). Rows start
// 16-byte aligned, so Q4_1 / Q5_1 blocks are whole aligned dwords; a Q5_0 block is 0 or 2 (mod 4)
// and takes the six dwords covering it, re-aligned with v_alignbyte as FmtQ0 does.
template <int T>
struct FmtQ1 {
    static constexpr bool KL = false;
    static constexpr int QKA = 32;
    static constexpr int ITEM = 32;
    static constexpr bool HAS_M = mi_type(T).has_m, HAS_QH = mi_type(T).has_qh;
    static constexpr bool Q50 = T == MI_TYPE_Q5_0;  // no m: the block is only 2-byte aligned
    static constexpr bool S1 = HAS_M;  // the activations' 16-bit slot: fp16 s (Q8_1), else the integer sum
    static constexpr int BS = mi_type(T).bytes;
    static constexpr int NW = HAS_QH ? 6 : 5;
    struct Regs {
        uint32_t w[NW];
        uint32_t off;  // Q5_0: byte offset of the block in w[0], 0 or 2
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        const uint32_t blk = (uint32_t) item * BS;
        r.off = Q50 ? blk & 2 : 0;
        const uint32_t base = blk - r.off;
#pragma unroll
        for (int i = 0; i < NW; i++) r.w[i] = *(const uint32_t *) (row + base + 4 * i);  // (Q5_0: 256 B tail slack)
    }
    // the block's levels as bytes (lo[i]: elements 4i.., hi[i]: elements 16 + 4i..) and its scales
    struct Blk {
        uint32_t lo[4], hi[4];
        float d, m;
    };
    __device__ static __forceinline__ void unpack(const Regs & r, Blk & b) {
        uint32_t qs[4], qh = 0;
        if constexpr (Q50) {
            b.d = mi_h2f((uint16_t) ((r.off ? r.w[0] >> 16 : r.w[0]) & 0xFFFF));
            b.m = 0.0f;
            qh = r.off ? r.w[1] : __builtin_amdgcn_alignbyte(r.w[1], r.w[0], 2);
#pragma unroll
            for (int i = 0; i < 4; i++) qs[i] = r.off ? r.w[i + 2] : __builtin_amdgcn_alignbyte(r.w[i + 2], r.w[i + 1], 2);
        } else {
            b.d = mi_h2f((uint16_t) (r.w[0] & 0xFFFF));
            b.m = mi_h2f((uint16_t) (r.w[0] >> 16));
            if constexpr (HAS_QH) qh = r.w[1];
#pragma unroll
            for (int i = 0; i < 4; i++) qs[i] = r.w[NW - 4 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            b.lo[i] = qs[i] & 0x0F0F0F0Fu;
            b.hi[i] = (qs[i] >> 4) & 0x0F0F0F0Fu;
            if constexpr (HAS_QH) {
                // four fifth bits to bit 4 of four bytes: bit k of x * 0x00204081 lands at k, k + 7,
                // k + 14, k + 21 (distinct, no carries); bits 0, 8, 16, 24 are kept
                b.lo[i] |= ((((qh >> (4 * i)) & 0xFu) * 0x00204081u) & 0x01010101u) << 4;
                b.hi[i] |= ((((qh >> (16 + 4 * i)) & 0xFu) * 0x00204081u) & 0x01010101u) << 4;
            }
        }
    }
    // tree order: the exact block integer (levels up to 31 fit mi_dot4's signed bytes), Q5_0 less
    // 16 sum(y); Q4_1 / Q5_1 add m * s with the fp16-rounded s
    __device__ static __forceinline__ float block_dot(const Blk & b, const int (&av)[8], int slot, float da, float acc) {
        int sumi = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sumi = mi_dot4((int) b.lo[i], av[i], sumi);
            sumi = mi_dot4((int) b.hi[i], av[i + 4], sumi);
        }
        if constexpr (!HAS_M) sumi -= 16 * slot;
        acc = fmaf((float) sumi, b.d * da, acc);
        if constexpr (HAS_M) acc = fmaf(b.m, mi_h2f((uint16_t) slot), acc);
        return acc;
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        Blk b;
        unpack(r, b);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 32);
            const int4 a0 = p[0], a1 = p[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            acc[c] = block_dot(b, av, (int) a.s32[c * (K / 32) + item], a.d[c * (K / 32) + item], acc[c]);
        }
    }
    struct Act {
        int av[8];
        int slot;
        float da;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) {
        const int4 * p = (const int4 *) (a.qs + (int64_t) item * 32);
        const int4 a0 = p[0], a1 = p[1];
        const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int i = 0; i < 8; i++) v.av[i] = av[i];
        v.slot = (int) a.s32[item];
        v.da = a.d[item];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int, const Act & v, float acc) {
        Blk b;
        unpack(r, b);
        return block_dot(b, v.av, v.slot, v.da, acc);
    }

    // CPU order (AVX2 ggml_vec_dot_q4_1_q8_1 src/ggml-quants.c:4006-4039, _q5_0_q8_0 :4279-4301,
    // _q5_1_q8_1 :4623-4648): eight f32 lanes, lane l = the exact int32 sum of q[e] y[e] over
    // e = 4l..4l+3 (Q5_0: q - 16), acc[l] = fma(x.d * y.d, (float) sum, acc[l]) over the blocks in
    // order; Q4_1 / Q5_1 also one scalar chain summs += x.m * y.s (the product of two fp16 values
    // is exact in f32, so a contracted fma gives the same bits). Scratch as FmtQ0's -- [l][slot], d
    // at [8][slot] -- plus the m s products at [9][slot].
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int S) {
        Blk b;
        unpack(r, b);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 32);
            const int4 a0 = p[0], a1 = p[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            uint32_t * e = scr + c * cs + slot;
#pragma unroll
            for (int l = 0; l < 8; l++) {
                const int lev = (int) (l < 4 ? b.lo[l & 3] : b.hi[l & 3]);
                const int q = HAS_M ? mi_dot4(lev, av[l], 0) : mi_dot4(lev, av[l], mi_dot4((int) 0xF0F0F0F0u, av[l], 0));  // (q - 16) . y
                e[l * S] = __float_as_uint((float) q);  // exact; _mm256_cvtepi32_ps
            }
            e[8 * S] = __float_as_uint(b.d * a.d[c * (K / 32) + item]);
            if constexpr (HAS_M) e[9 * S] = __float_as_uint(b.m * mi_h2f((uint16_t) a.s32[c * (K / 32) + item]));
        }
    }
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int S, float & A, float & M) {
        if constexpr (!HAS_M) {
            FmtQ0<true>::chain(scr, l, n_items, S, A, M);
        } else {
            // the lane's fma chain and summs (in block order) side by side: two independent chains
            const float * q = (const float *) scr + l * S;
            const float * d = (const float *) scr + 8 * S;
            const float * ms = (const float *) scr + 9 * S;
            int i = 0;
            for (; i + 4 <= n_items; i += 4) {
                const float4 qq = *(const float4 *) (q + i);
                const float4 dd = *(const float4 *) (d + i);
                const float4 mm = *(const float4 *) (ms + i);
                A = fmaf(dd.x, qq.x, A);
                M = M + mm.x;
                A = fmaf(dd.y, qq.y, A);
                M = M + mm.y;
                A = fmaf(dd.z, qq.z, A);
                M = M + mm.z;
                A = fmaf(dd.w, qq.w, A);
                M = M + mm.w;
            }
            for (; i < n_items; i++) {
                A = fmaf(d[i], q[i], A);
                M = M + ms[i];
            }
        }
    }
    static int ord_words(int nitems, int & stride) {
        const int w = FmtQ0<true>::ord_words(nitems, stride);
        return HAS_M ? w / 9 * 10 : w;
    }
    __device__ static __forceinline__ float finish(float A, float M) {
        const float z = FmtQ0<true>::finish(A, 0.0f);
        return HAS_M ? z + M : z;  // hsum_float_8(acc) + summs
    }
};

// Q4_0 in pairs of blocks (tree order only): an item is 2 blocks = 36 B, 4-byte aligned, so 9
// dword loads cover it with no slack, the second block's quants are whole dwords (only the
// first's need v_alignbyte), and a K = 4096 row is one item per lane.
// one pair of Q4_0 blocks against its q8_0 activations: block quants t0 / t1 (16 bytes each), scales
// dw0 / dw1; shared by FmtQ0Pair and FmtQ0R, so the canonical and the repacked layouts give the
// same bits
__device__ __forceinline__ float q0pair_dot(const uint32_t (&t0)[4], const uint32_t (&t1)[4], float dw0, float dw1, const int (&av0)[8],
                                            const int (&av1)[8], uint32_t ss, float2 da, float acc) {
    int s0 = 0, s1 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s0 = mi_dot4((int) (t0[i] & 0x0F0F0F0Fu), av0[i], s0);
        s0 = mi_dot4((int) ((t0[i] >> 4) & 0x0F0F0F0Fu), av0[i + 4], s0);
        s1 = mi_dot4((int) (t1[i] & 0x0F0F0F0Fu), av1[i], s1);
        s1 = mi_dot4((int) ((t1[i] >> 4) & 0x0F0F0F0Fu), av1[i + 4], s1);
    }
    s0 -= 8 * (int) (int16_t) (ss & 0xFFFF);
    s1 -= 8 * (int) (int16_t) (ss >> 16);
    acc = fmaf((float) s0, dw0 * da.x, acc);
    return fmaf((float) s1, dw1 * da.y, acc);
}

struct FmtQ0Pair {
    static constexpr bool KL = false;
    static constexpr int QKA = 32;
    static constexpr int ITEM = 64;
    struct Regs {
        uint32_t w[9];
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        const uint8_t * p = row + (uint32_t) item * 36;
#pragma unroll
        for (int i = 0; i < 9; i++) r.w[i] = *(const uint32_t *) (p + 4 * i);
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        // block 0: d = bytes 0..1, quants bytes 2..17; block 1: d = bytes 18..19, quants 20..35
        uint32_t t0[4];
#pragma unroll
        for (int i = 0; i < 4; i++) t0[i] = __builtin_amdgcn_alignbyte(r.w[i + 1], r.w[i], 2);
        const float dw0 = mi_h2f((uint16_t) (r.w[0] & 0xFFFF));
        const float dw1 = mi_h2f((uint16_t) (r.w[4] >> 16));
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 64);
            const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
            const int av0[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const int av1[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            const uint32_t ss = *(const uint32_t *) (a.s32 + c * (K / 32) + 2 * item);  // both blocks' sums
            const float2 da = *(const float2 *) (a.d + c * (K / 32) + 2 * item);
            acc[c] = pair_dot(r, t0, dw0, dw1, av0, av1, ss, da, acc[c]);
        }
    }
    __device__ static __forceinline__ float pair_dot(const Regs & r, const uint32_t (&t0)[4], float dw0, float dw1, const int (&av0)[8],
                                                     const int (&av1)[8], uint32_t ss, float2 da, float acc) {
        const uint32_t t1[4] = {r.w[5], r.w[6], r.w[7], r.w[8]};
        return q0pair_dot(t0, t1, dw0, dw1, av0, av1, ss, da, acc);
    }
    struct Act {
        int av0[8], av1[8];
        uint32_t ss;
        float2 da;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) {
        const int4 * p = (const int4 *) (a.qs + (int64_t) item * 64);
        const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
        const int av0[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const int av1[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            v.av0[i] = av0[i];
            v.av1[i] = av1[i];
        }
        v.ss = *(const uint32_t *) (a.s32 + 2 * item);
        v.da = *(const float2 *) (a.d + 2 * item);
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int, const Act & v, float acc) {
        uint32_t t0[4];
#pragma unroll
        for (int i = 0; i < 4; i++) t0[i] = __builtin_amdgcn_alignbyte(r.w[i + 1], r.w[i], 2);
        return pair_dot(r, t0, mi_h2f((uint16_t) (r.w[0] & 0xFFFF)), mi_h2f((uint16_t) (r.w[4] >> 16)), v.av0, v.av1, v.ss, v.da, acc);
    }
};

// Q4_0 block pairs on the 16-byte-aligned repacked copy (tree order only; mmq_planes.hip
// k_q40_repack): per row [K/32 blocks x 16 quant bytes][K/32 x f16 d], so item (pair) p is two
// aligned dwordx4 at 32 p and one dword at K/2 + 4 p -- consecutive lanes read consecutive bytes.
// The same pair arithmetic as FmtQ0Pair (q0pair_dot): bit-identical outputs.
struct FmtQ0R {
    static constexpr bool KL = true;  // load() needs K (the scales follow the row's quants)
    static constexpr int QKA = 32;
    static constexpr int ITEM = 64;
    struct Regs {
        uint4 q0, q1;
        uint32_t d;
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item, int64_t K) {
        const uint32_t o = (uint32_t) item * 32;
        r.q0 = *(const uint4 *) (row + o);
        r.q1 = *(const uint4 *) (row + o + 16);
        r.d = *(const uint32_t *) (row + (uint32_t) (K / 2) + 4 * (uint32_t) item);
    }
    __device__ static __forceinline__ float pdot(const Regs & r, const int (&av0)[8], const int (&av1)[8], uint32_t ss, float2 da, float acc) {
        const uint32_t t0[4] = {r.q0.x, r.q0.y, r.q0.z, r.q0.w};
        const uint32_t t1[4] = {r.q1.x, r.q1.y, r.q1.z, r.q1.w};
        return q0pair_dot(t0, t1, mi_h2f((uint16_t) (r.d & 0xFFFF)), mi_h2f((uint16_t) (r.d >> 16)), av0, av1, ss, da, acc);
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 64);
            const int4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
            const int av0[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const int av1[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            const uint32_t ss = *(const uint32_t *) (a.s32 + c * (K / 32) + 2 * item);
            const float2 da = *(const float2 *) (a.d + c * (K / 32) + 2 * item);
            acc[c] = pdot(r, av0, av1, ss, da, acc[c]);
        }
    }
    using Act = FmtQ0Pair::Act;
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) { FmtQ0Pair::act_load(v, item, a, K); }
    __device__ static __forceinline__ float dot_act(const Regs & r, int, const Act & v, float acc) { return pdot(r, v.av0, v.av1, v.ss, v.da, acc); }
};

// Q8_0 blocks on the 16-byte-aligned repacked copy (tree order only; k_q80_repack): per row [K/32
// blocks x 32 quant bytes][K/32 x f16 d], item = one block as for FmtQ0<true> (lane l: blocks l,
// l + 64, ...) with FmtQ0<true>'s arithmetic (block_dot): bit-identical outputs. A lane's block is
// two aligned dwordx4; its scale comes with its neighbour's in one dword (selected by parity).
struct FmtQ8R {
    static constexpr bool KL = true;
    static constexpr int QKA = 32;
    static constexpr int ITEM = 32;
    using Q = FmtQ0<true>;
    struct Regs {
        uint4 q0, q1;
        uint32_t dd;
        uint32_t odd;  // 16 if the item is odd (its d in the high half of dd)
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item, int64_t K) {
        const uint32_t o = (uint32_t) item * 32;
        r.q0 = *(const uint4 *) (row + o);
        r.q1 = *(const uint4 *) (row + o + 16);
        r.dd = *(const uint32_t *) (row + (uint32_t) K + 4 * ((uint32_t) item >> 1));
        r.odd = ((uint32_t) item & 1) * 16;
    }
    __device__ static __forceinline__ float bdot(const Regs & r, const int (&av)[8], float da, float acc) {
        const uint32_t t[8] = {r.q0.x, r.q0.y, r.q0.z, r.q0.w, r.q1.x, r.q1.y, r.q1.z, r.q1.w};
        return Q::block_dot(t, mi_h2f((uint16_t) ((r.dd >> r.odd) & 0xFFFF)), av, 0, da, acc);
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            const int4 * p = (const int4 *) (a.qs + c * K + (int64_t) item * 32);
            const int4 a0 = p[0], a1 = p[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            acc[c] = bdot(r, av, a.d[c * (K / 32) + item], acc[c]);
        }
    }
    using Act = Q::Act;
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t K) { Q::act_load(v, item, a, K); }
    __device__ static __forceinline__ float dot_act(const Regs & r, int, const Act & v, float acc) { return bdot(r, v.av, v.da, acc); }
};

// Q6_K (210 B superblocks: ql[128] | qh[64] | int8 scales[16] | fp16 d; element e is
// d * scales[e / 16] * (q - 32)). An item is (superblock s, 128-half h, 16-byte range u), item =
// 4 s + 2 h + u: ql[64h + 16u ..], ql[64h + 32 + 16u ..] and qh[32h + 16u ..] hold the four
// 16-element sub-blocks at elements 128h + 32t + 16u (t = 0..3; t & 1 picks the ql range, t & 2 its
// high nibbles, qh bits 2t..2t+1 the upper two bits), whose scales are scales[8h + 2t + u]. Four
// items per superblock on adjacent lanes, so a K = 4096 row is one item per lane, as Q4_K.
// Blocks are 2-byte aligned and so are rows of an odd superblock count (LLaMA's ffn_down,
// K = 11008: 9030-byte rows), so the misalignment of a block is taken from its address: every load
// is an aligned dword from two bytes below or at the data, re-aligned with v_alignbyte (shift 0 or
// 2). The dword after a 16-byte range still lies in the block; the one holding d may reach two
// bytes past it (the next block, or the buffer's tail slack).
struct FmtQ6K {
    static constexpr bool KL = false;
    static constexpr int QKA = 256;
    static constexpr int ITEM = 64;
    static constexpr int BS = mi_type(MI_TYPE_Q6_K).bytes;
    struct Regs {
        uint32_t la[5], lb[5], hh[5];  // the dwords covering the two ql ranges and the qh range
        uint32_t sc[3];                // ... the eight scales of the 128-half
        uint32_t dd;                   // ... d
        uint32_t off;                  // the block's misalignment: 0 or 2
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        const uint32_t s = (uint32_t) item >> 2, h = ((uint32_t) item >> 1) & 1, u = (uint32_t) item & 1;
        const uint32_t blk = s * BS;
        r.off = ((uint32_t) (uintptr_t) row + blk) & 2;
        const uint8_t * p = row + (int) (blk - r.off);  // 4-byte aligned (item 0 of a misaligned row: its first dword starts in the row before)
        const uint32_t qa = 64 * h + 16 * u, qh = 128 + 32 * h + 16 * u, sc = 192 + 8 * h;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            r.la[i] = *(const uint32_t *) (p + qa + 4 * i);
            r.lb[i] = *(const uint32_t *) (p + qa + 32 + 4 * i);
            r.hh[i] = *(const uint32_t *) (p + qh + 4 * i);
        }
        r.sc[0] = *(const uint32_t *) (p + sc);
        r.sc[1] = *(const uint32_t *) (p + sc + 4);
        r.sc[2] = *(const uint32_t *) (p + sc + (r.off ? 8 : 4));  // (aligned blocks: not needed, no read past d)
        r.dd = *(const uint32_t *) (p + 208);
    }
    // the item's operands: (q - 32) of sub-block t as four int8x4 dwords, its scale, the block's d
    struct Dec {
        int q[4][4];
        int sc[4];
        float dw;
    };
    // bytes of q (each 0..63) -> bytes of q - 32 as int8, no carries between the bytes
    __device__ static __forceinline__ int center(uint32_t q) { return (int) (((q | 0x80808080u) - 0x20202020u) ^ 0x80808080u); }
    __device__ static __forceinline__ void decode(Dec & d, const Regs & r, int item) {
        const int u = item & 1;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t la = __builtin_amdgcn_alignbyte(r.la[i + 1], r.la[i], r.off);
            const uint32_t lb = __builtin_amdgcn_alignbyte(r.lb[i + 1], r.lb[i], r.off);
            const uint32_t hh = __builtin_amdgcn_alignbyte(r.hh[i + 1], r.hh[i], r.off);
            d.q[0][i] = center((la & 0x0F0F0F0Fu) | ((hh & 0x03030303u) << 4));
            d.q[1][i] = center((lb & 0x0F0F0F0Fu) | (((hh >> 2) & 0x03030303u) << 4));
            d.q[2][i] = center(((la >> 4) & 0x0F0F0F0Fu) | (((hh >> 4) & 0x03030303u) << 4));
            d.q[3][i] = center(((lb >> 4) & 0x0F0F0F0Fu) | (((hh >> 6) & 0x03030303u) << 4));
        }
        const uint32_t s0 = __builtin_amdgcn_alignbyte(r.sc[1], r.sc[0], r.off) >> (8 * u);
        const uint32_t s1 = __builtin_amdgcn_alignbyte(r.sc[2], r.sc[1], r.off) >> (8 * u);
        d.sc[0] = (int) (int8_t) (s0 & 0xFF);
        d.sc[1] = (int) (int8_t) ((s0 >> 16) & 0xFF);
        d.sc[2] = (int) (int8_t) (s1 & 0xFF);
        d.sc[3] = (int) (int8_t) ((s1 >> 16) & 0xFF);
        d.dw = mi_h2f((uint16_t) ((r.dd >> (8 * r.off)) & 0xFFFF));
    }
    // the item's 64 quantized activations of one column: sub-block t = av[4t .. 4t+3]
    __device__ static __forceinline__ void act16(int (&av)[16], const int8_t * qs, int item) {
        const int s = item >> 2, h = (item >> 1) & 1, u = item & 1;
        const int4 * p = (const int4 *) (qs + (int64_t) s * 256 + 128 * h + 16 * u);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int4 a = p[2 * t];
            av[4 * t] = a.x; av[4 * t + 1] = a.y; av[4 * t + 2] = a.z; av[4 * t + 3] = a.w;
        }
    }
    // An item's integer sum can reach 4 * 128 * 16 * 32 * 128 = 2^25, which f32 does not hold
    // exactly (FmtKQ's f32 scale products do not carry over): int32, converted once.
    __device__ static __forceinline__ float item_dot(const Dec & d, const int (&av)[16], float ad, float acc) {
        int sumi = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int p = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) p = mi_dot4(d.q[t][i], av[4 * t + i], p);
            sumi += __mul24(d.sc[t], p);  // |p| <= 16 * 32 * 128
        }
        return fmaf((float) sumi, d.dw * ad, acc);
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        Dec d;
        decode(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16];
            act16(av, a.qs + c * K, item);
            acc[c] = item_dot(d, av, a.d[c * (K / 256) + (item >> 2)], acc[c]);
        }
    }
    struct Act {
        int av[16];
        float ad;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t) {
        act16(v.av, a.qs, item);
        v.ad = a.d[item >> 2];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int item, const Act & v, float acc) {
        Dec d;
        decode(d, r, item);
        return item_dot(d, v.av, v.ad, acc);
    }

    // CPU order (ggml_vec_dot_q6_K_q8_K, AVX2): eight int32 lanes per superblock, lane l = sum over
    // the eight 32-groups g of scales[2g + (l >= 4)] * sum_{e = 4l..4l+3} (q - 32)[32g + e] a[32g + e].
    // Item (h, u) holds groups g = 4h + t at bytes 16u..16u+15, i.e. CPU lanes 4u + i (its dword i)
    // with exactly its four scales; the two h items of the quad add up to the lane totals (< 2^24 in
    // magnitude, or exactly 2^24: the float conversion is exact). Entry of superblock sb in the
    // scratch: [0..7] the eight sums as floats, [12] d = y.d * x.d (FmtKQ's slots).
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int) {
        const int h = (item >> 1) & 1, u = item & 1;
        Dec d;
        decode(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16];
            act16(av, a.qs + c * K, item);
            int v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = 0;
#pragma unroll
                for (int t = 0; t < 4; t++) v[i] += __mul24(d.sc[t], mi_dot4(d.q[t][i], av[4 * t + i], 0));
                v[i] += mi_dpp<MI_DPP_QP_2301>(0, v[i]);  // the other 128-half: lane ^ 2 of the quad
            }
            uint32_t * e = scr + c * cs + (slot >> 2) * 16;
            if (h == 0) {
                *(uint4 *) (e + 4 * u) = make_uint4(__float_as_uint((float) v[0]), __float_as_uint((float) v[1]),
                                                   __float_as_uint((float) v[2]), __float_as_uint((float) v[3]));
            } else if (u == 0) {
                e[12] = __float_as_uint(a.d[c * (K / 256) + (item >> 2)] * d.dw);
            }
        }
    }
    // acc[l] = fma(d, (float) sumi[l], acc[l]) per superblock (_mm256_fmadd_ps)
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int, float & A, float &) {
        const float * e = (const float *) scr;
        const int nsb = n_items >> 2;
        for (int sb = 0; sb < nsb; sb++, e += 16) A = fmaf(e[12], e[l], A);
    }
    static int ord_words(int nitems, int & stride) {
        stride = 0;
        return 16 * (nitems / 4) + 8;
    }
    __device__ static __forceinline__ float finish(float A, float) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A + __shfl_xor(A, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        return z + __shfl_xor(z, 1, 8);
    }
};

// Q2_K (84 B superblocks: scales[16] | qs[64] | fp16 d | fp16 dmin; element d (sc & 0xF) q -
// dmin (sc >> 4)) and Q3_K (110 B: hmask[32] | qs[64] | scales[12] | fp16 d; element
// d (sc - 32) (q - (hbit ? 0 : 4)), sc the 6-bit scale of the kmask1 / kmask2 unpack). Both pack
// the quants as Q6_K packs its ql halves -- byte qs[32h + b] holds at bit 2t element 128h + 32t + b,
// and bit 4h + t of hmask[b] is that element's high bit -- so FmtQ6K's item serves both: (superblock
// s, 128-half h, 16-byte range u), item = 4 s + 2 h + u, reads qs[32h + 16u ..+15] (Q3_K: and
// hmask[16u ..+15]), i.e. the four 16-element sub-blocks at elements 128h + 32t + 16u (t = 0..3) with
// scales index 8h + 2t + u. Four items per superblock on adjacent lanes; a K = 4096 row is one item
// per lane.
// Loads: Q2_K blocks are 4-byte aligned wherever the row is (84 = 4 * 21), so its seven dwords
// (four of quants, the eight scale bytes of the 128-half, d | dmin) are read where they lie. Q3_K
// blocks are 2-byte aligned and rows of an odd superblock count are 2 mod 4 (K = 11008: 4730-byte
// rows): as FmtQ6K, every load is an aligned dword from two bytes below or at the data, re-aligned
// with v_alignbyte by the block's own misalignment. The dword that holds d of an aligned block
// reaches two bytes past the block (the next block, or the buffer's tail slack); nothing reaches
// further.
// Q2_K's mins need the 16-element sums of the Q8_K activations, which the activations in LDS do
// not keep (s32: sums of 32): v_dot4 of the quants in hand against 0x01010101 -- at one column in
// tree order once per kernel (Act), not per row.
template <bool Q3>
struct FmtQ23K {
    static constexpr bool KL = false;
    static constexpr int QKA = 256;
    static constexpr int ITEM = 64;
    static constexpr int BS = mi_type(Q3 ? MI_TYPE_Q3_K : MI_TYPE_Q2_K).bytes;
    static constexpr int E = Q3 ? 16 : 20;  // scratch words per superblock in the reference order
    struct Regs {
        uint32_t qs[Q3 ? 5 : 4];  // the dwords covering the 16 quant bytes
        uint32_t hm[Q3 ? 5 : 1];  // Q3_K: ... the 16 hmask bytes
        uint32_t sc[Q3 ? 4 : 2];  // Q3_K: the 12 scale bytes and d; Q2_K: the eight scales | mins of the 128-half
        uint32_t dd;              // Q2_K: d | dmin; Q3_K: the block's misalignment, 0 or 2
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        const uint32_t s = (uint32_t) item >> 2, h = ((uint32_t) item >> 1) & 1, u = (uint32_t) item & 1;
        const uint32_t blk = s * BS;
        if constexpr (Q3) {
            const uint32_t off = ((uint32_t) (uintptr_t) row + blk) & 2;
            r.dd = off;
            const uint8_t * p = row + (int) (blk - off);  // 4-byte aligned (item 0 of a misaligned row: its first dword starts in the row before)
#pragma unroll
            for (int i = 0; i < 5; i++) {
                r.hm[i] = *(const uint32_t *) (p + 16 * u + 4 * i);
                r.qs[i] = *(const uint32_t *) (p + 32 + 32 * h + 16 * u + 4 * i);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) r.sc[i] = *(const uint32_t *) (p + 96 + 4 * i);  // scales, and d in sc[3]
        } else {
            const uint8_t * p = row + blk;
#pragma unroll
            for (int i = 0; i < 4; i++) r.qs[i] = *(const uint32_t *) (p + 16 + 32 * h + 16 * u + 4 * i);
            r.hm[0] = 0u;
            r.sc[0] = *(const uint32_t *) (p + 8 * h);
            r.sc[1] = *(const uint32_t *) (p + 8 * h + 4);
            r.dd = *(const uint32_t *) (p + 80);
        }
    }
    // the item's operands: sub-block t's levels (Q2_K q, Q3_K q - 4 * !hbit) as four int8x4 dwords,
    // its scale (Q2_K sc & 0xF, Q3_K sc - 32) and min, the block's d and dmin
    struct Dec {
        int q[4][4];
        int sc[4];
        int mn[Q3 ? 1 : 4];
        float dw, dmw;
    };
    // CENTER (Q3_K): the levels as q - 4 * !hbit in -4..3; else as v = q | hbit << 2 in 0..7, for
    // callers that take the 4 off on the activations' side, dot(v - 4, a) = dot(v, a) - 4 sum(a)
    // (nine VALU operations per dword and sub-block become four: the streaming kernel at one column
    // was bound by them, not by HBM)
    template <bool CENTER = true>
    __device__ static __forceinline__ void decode(Dec & d, const Regs & r, int item) {
        const uint32_t h = ((uint32_t) item >> 1) & 1, u = (uint32_t) item & 1;
        if constexpr (Q3) {
            const uint32_t off = r.dd;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t qs = __builtin_amdgcn_alignbyte(r.qs[i + 1], r.qs[i], off);
                const uint32_t hb = (__builtin_amdgcn_alignbyte(r.hm[i + 1], r.hm[i], off) >> (4 * h)) << 2;  // high bit of sub-block t at bit 2 + t
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const uint32_t v = ((qs >> (2 * t)) & 0x03030303u) | ((hb >> t) & 0x04040404u);
                    // v - 4 per byte, no carries: (v + 128 - 4) never borrows, the xor takes the 128 back out
                    d.q[t][i] = CENTER ? (int) (((v | 0x80808080u) - 0x04040404u) ^ 0x80808080u) : (int) v;
                }
            }
            // scales j = 8h + 2t + u: low nibbles in byte 2t + u of aux[0..1] (nibble h), upper two bits in
            // byte 2 (t & 1) + u of aux[2] at bit 2 (2h + (t >> 1))
            const uint32_t sh = 8 * u + 4 * h;
            const uint32_t x0 = __builtin_amdgcn_alignbyte(r.sc[1], r.sc[0], off) >> sh;
            const uint32_t x1 = __builtin_amdgcn_alignbyte(r.sc[2], r.sc[1], off) >> sh;
            const uint32_t y = __builtin_amdgcn_alignbyte(r.sc[3], r.sc[2], off) >> sh;
            d.sc[0] = (int) ((x0 & 0xF) | ((y & 3) << 4)) - 32;
            d.sc[1] = (int) (((x0 >> 16) & 0xF) | (((y >> 16) & 3) << 4)) - 32;
            d.sc[2] = (int) ((x1 & 0xF) | (((y >> 2) & 3) << 4)) - 32;
            d.sc[3] = (int) (((x1 >> 16) & 0xF) | (((y >> 18) & 3) << 4)) - 32;
            d.mn[0] = 0;
            d.dw = mi_h2f((uint16_t) ((r.sc[3] >> (8 * off)) & 0xFFFF));
            d.dmw = 0.0f;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int t = 0; t < 4; t++) d.q[t][i] = (int) ((r.qs[i] >> (2 * t)) & 0x03030303u);
            }
            const uint32_t x0 = r.sc[0] >> (8 * u), x1 = r.sc[1] >> (8 * u);
            d.sc[0] = (int) (x0 & 0xF);         d.mn[0] = (int) ((x0 >> 4) & 0xF);
            d.sc[1] = (int) ((x0 >> 16) & 0xF); d.mn[1] = (int) ((x0 >> 20) & 0xF);
            d.sc[2] = (int) (x1 & 0xF);         d.mn[2] = (int) ((x1 >> 4) & 0xF);
            d.sc[3] = (int) ((x1 >> 16) & 0xF); d.mn[3] = (int) ((x1 >> 20) & 0xF);
            d.dw = mi_h2f((uint16_t) (r.dd & 0xFFFF));
            d.dmw = mi_h2f((uint16_t) (r.dd >> 16));
        }
    }
    // the item's 64 quantized activations of one column: sub-block t = av[4t .. 4t+3]
    __device__ static __forceinline__ void act16(int (&av)[16], const int8_t * qs, int item) {
        const int s = item >> 2, h = (item >> 1) & 1, u = item & 1;
        const int4 * p = (const int4 *) (qs + (int64_t) s * 256 + 128 * h + 16 * u);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int4 a = p[2 * t];
            av[4 * t] = a.x; av[4 * t + 1] = a.y; av[4 * t + 2] = a.z; av[4 * t + 3] = a.w;
        }
    }
    // the sum of sub-block t's 16 quants: bsums[8h + 2t + u] of the column's Q8_K block
    __device__ static __forceinline__ int sum16(const int (&av)[16], int t) {
        int b = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) b = mi_dot4(0x01010101, av[4 * t + i], b);
        return b;
    }
    // every integer below is exact in f32: an item's sum is at most 4 * 16 * 4 * 128 * 32 = 2^20, its
    // mins sum at most 4 * 15 * 16 * 128 < 2^17
    template <bool CENTER = true>
    __device__ static __forceinline__ float item_dot(const Dec & d, const int (&av)[16], const int (&b16)[4], float ad, float acc) {
        int sumi = 0, summ = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int p = Q3 && !CENTER ? -4 * b16[t] : 0;
#pragma unroll
            for (int i = 0; i < 4; i++) p = mi_dot4(d.q[t][i], av[4 * t + i], p);
            sumi += __mul24(d.sc[t], p);
            if constexpr (!Q3) summ += __mul24(d.mn[t], b16[t]);
        }
        if constexpr (Q3) return fmaf((float) sumi, d.dw * ad, acc);
        // explicit fmas (the file contracts freely): the same bits in every kernel that inlines this
        else return fmaf(ad, fmaf(-d.dmw, (float) summ, d.dw * (float) sumi), acc);
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        // Q3_K at one column: the 16 sums cost less than centering the 16 dwords of levels
        constexpr bool CENTER = NC > 1;
        Dec d;
        decode<CENTER>(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16], b16[4] = {0, 0, 0, 0};
            act16(av, a.qs + c * K, item);
            if constexpr (!Q3 || !CENTER) {
#pragma unroll
                for (int t = 0; t < 4; t++) b16[t] = sum16(av, t);
            }
            acc[c] = item_dot<CENTER>(d, av, b16, a.d[c * (K / 256) + (item >> 2)], acc[c]);
        }
    }
    struct Act {
        int av[16];
        int b16[4];
        float ad;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t) {
        act16(v.av, a.qs, item);
#pragma unroll
        for (int t = 0; t < 4; t++) v.b16[t] = sum16(v.av, t);
        v.ad = a.d[item >> 2];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int item, const Act & v, float acc) {
        Dec d;
        decode<false>(d, r, item);
        return item_dot<false>(d, v.av, v.b16, v.ad, acc);
    }

    // CPU order (ggml_vec_dot_q2_K_q8_K / _q3_K_q8_K, AVX2): eight int32 lanes per superblock, lane l =
    // sum over the eight 32-groups g of S[2g + (l >= 4)] * sum_{e = 4l..4l+3} Q[32g + e] a[32g + e].
    // Item (h, u) holds groups g = 4h + t at bytes 16u..16u+15, i.e. CPU lanes 4u + i (its dword i)
    // with exactly its four scales; the two h items of the quad add up to the lane totals (at most
    // 2^19). Q2_K's mins lane l is m[2l] bsums[2l] + m[2l+1] bsums[2l+1]: sub-blocks 8h + 2t + u of the
    // items (h, 0) and (h, 1) with l = 4h + t, which add up over the u pair. Entry of superblock sb
    // in the scratch, E words: [0..7] the eight sums as floats; Q3_K [12] d = y.d * x.d (FmtKQ's
    // slot); Q2_K [8..15] the eight mins lanes, [16] d, [17] dmin = -(y.d * x.dmin).
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int) {
        const int h = (item >> 1) & 1, u = item & 1;
        constexpr bool CENTER = NC > 1;  // Q3_K at one column: a second v_dot4 against -4 instead of centering
        Dec d;
        decode<CENTER>(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16];
            act16(av, a.qs + c * K, item);
            int v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                v[i] = 0;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int off4 = Q3 && !CENTER ? mi_dot4((int) 0xFCFCFCFCu, av[4 * t + i], 0) : 0;
                    v[i] += __mul24(d.sc[t], mi_dot4(d.q[t][i], av[4 * t + i], off4));
                }
                v[i] += mi_dpp<MI_DPP_QP_2301>(0, v[i]);  // the other 128-half: lane ^ 2 of the quad
            }
            uint32_t * e = scr + c * cs + (slot >> 2) * E;
            const float yd = a.d[c * (K / 256) + (item >> 2)];
            if constexpr (!Q3) {
                int pm[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    pm[t] = __mul24(d.mn[t], sum16(av, t));
                    pm[t] += mi_dpp<MI_DPP_QP_1032>(0, pm[t]);  // the other 16-byte range: lane ^ 1 of the quad
                }
                if (u == 0) {
                    *(uint4 *) (e + 8 + 4 * h) = make_uint4(__float_as_uint((float) pm[0]), __float_as_uint((float) pm[1]),
                                                           __float_as_uint((float) pm[2]), __float_as_uint((float) pm[3]));
                } else if (h == 1) {
                    *(uint2 *) (e + 16) = make_uint2(__float_as_uint(yd * d.dw), __float_as_uint(-(yd * d.dmw)));
                }
            }
            if (h == 0) {
                *(uint4 *) (e + 4 * u) = make_uint4(__float_as_uint((float) v[0]), __float_as_uint((float) v[1]),
                                                   __float_as_uint((float) v[2]), __float_as_uint((float) v[3]));
            } else if (Q3 && u == 0) {
                e[12] = __float_as_uint(yd * d.dw);
            }
        }
    }
    // per superblock: Q2_K acc[l] = fma(dmin, (float) mins[l], acc[l]) first, then for both
    // acc[l] = fma(d, (float) sumi[l], acc[l]) (_mm256_fmadd_ps)
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int, float & A, float &) {
        const float * e = (const float *) scr;
        const int nsb = n_items >> 2;
        for (int sb = 0; sb < nsb; sb++, e += E) {
            if constexpr (Q3) {
                A = fmaf(e[12], e[l], A);
            } else {
                A = fmaf(e[17], e[8 + l], A);
                A = fmaf(e[16], e[l], A);
            }
        }
    }
    static int ord_words(int nitems, int & stride) {
        stride = 0;
        return E * (nitems / 4) + 8;
    }
    __device__ static __forceinline__ float finish(float A, float) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A + __shfl_xor(A, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        return z + __shfl_xor(z, 1, 8);
    }
};
using FmtQ2K = FmtQ23K<false>;
using FmtQ3K = FmtQ23K<true>;

// IQ4_XS (136 B superblocks: fp16 d | u16 scales_h | scales_l[4] | qs[128]; sub-block ib of 32
// elements has its quants at qs[16 ib ..], element j < 16 the low nibble of byte j and element 16 + j
// its high nibble, both indices into kvalues_iq4nl, and the 6-bit scale ls = nibble ib of scales_l |
// bits 2 ib.. of scales_h << 4; element value d (ls - 32) kvalues[q]). Item (superblock s, quarter u),
// item = 4 s + u: the 8-byte header and qs[32u .. 32u + 31], i.e. the sub-blocks 2u and 2u + 1 and 64
// activations. Four items per superblock on adjacent lanes; a K = 4096 row is one item per lane.
// Loads: blocks are 8-byte aligned wherever the row lies (136 = 8 * 17; rows of an odd superblock
// count are 8 mod 16, K = 11008: 5848 bytes), so the item is five aligned 8-byte words of its own
// block: nothing is read outside the block.
// The levels are looked up once per item (mi_iq4nl_levels) and used for every column.
struct FmtIQ4XS {
    static constexpr bool KL = false;
    static constexpr int QKA = 256;
    static constexpr int ITEM = 64;
    static constexpr int BS = mi_type(MI_TYPE_IQ4_XS).bytes;
    static constexpr int E = 16;  // scratch words per superblock in the reference order
    struct Regs {
        uint2 hdr;   // d | scales_h << 16, scales_l
        uint2 q[4];  // the 32 quant bytes
    };
    __device__ static __forceinline__ void load(Regs & r, const uint8_t * row, int item) {
        const uint32_t s = (uint32_t) item >> 2, u = (uint32_t) item & 3;
        const uint8_t * p = row + s * BS;
        r.hdr = *(const uint2 *) p;
#pragma unroll
        for (int i = 0; i < 4; i++) r.q[i] = *(const uint2 *) (p + 8 + 32 * u + 8 * i);
    }
    // the item's operands: lv[0..7] the levels of sub-block 2u (lv[l]: its elements 4l..4l+3, the
    // reference's lane l), lv[8..15] those of sub-block 2u + 1, their scales minus 32, the block's d
    struct Dec {
        int lv[16];
        int ls0, ls1;
        float dw;
    };
    __device__ static __forceinline__ void decode(Dec & d, const Regs & r, int item) {
        const uint32_t u = (uint32_t) item & 3;
        const uint32_t sh = r.hdr.x >> (16 + 4 * u), sl = r.hdr.y >> (8 * u);
        d.dw = mi_h2f((uint16_t) (r.hdr.x & 0xFFFF));
        d.ls0 = (int) ((sl & 0xF) | ((sh & 3) << 4)) - 32;
        d.ls1 = (int) (((sl >> 4) & 0xF) | (((sh >> 2) & 3) << 4)) - 32;
        const uint32_t q[8] = {r.q[0].x, r.q[0].y, r.q[1].x, r.q[1].y, r.q[2].x, r.q[2].y, r.q[3].x, r.q[3].y};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            mi_iq4nl_levels8(q[i], d.lv[i], d.lv[4 + i]);
            mi_iq4nl_levels8(q[4 + i], d.lv[8 + i], d.lv[12 + i]);
        }
    }
    // the item's 64 quantized activations of one column
    __device__ static __forceinline__ void act16(int (&av)[16], const int8_t * qs, int item) {
        const int4 * p = (const int4 *) (qs + (int64_t) (item >> 2) * 256 + 64 * (item & 3));
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int4 a = p[t];
            av[4 * t] = a.x; av[4 * t + 1] = a.y; av[4 * t + 2] = a.z; av[4 * t + 3] = a.w;
        }
    }
    // a sub-block's scaled sum is below 32 * 127 * 127 * 32 < 2^24: exact in f32
    __device__ static __forceinline__ float item_dot(const Dec & d, const int (&av)[16], float ad, float acc) {
        int p0 = 0, p1 = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            p0 = mi_dot4(d.lv[i], av[i], p0);
            p1 = mi_dot4(d.lv[8 + i], av[8 + i], p1);
        }
        // explicit fmas (the file contracts freely): the same bits in every kernel that inlines this
        const float dd = d.dw * ad;
        return fmaf((float) (d.ls1 * p1), dd, fmaf((float) (d.ls0 * p0), dd, acc));
    }
    template <int NC>
    __device__ static __forceinline__ void dot(const Regs & r, int item, const lds_act & a, int64_t K, int ncols, float (&acc)[NC]) {
        Dec d;
        decode(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16];
            act16(av, a.qs + c * K, item);
            acc[c] = item_dot(d, av, a.d[c * (K / 256) + (item >> 2)], acc[c]);
        }
    }
    struct Act {
        int av[16];
        float ad;
    };
    __device__ static __forceinline__ void act_load(Act & v, int item, const lds_act & a, int64_t) {
        act16(v.av, a.qs, item);
        v.ad = a.d[item >> 2];
    }
    __device__ static __forceinline__ float dot_act(const Regs & r, int item, const Act & v, float acc) {
        Dec d;
        decode(d, r, item);
        return item_dot(d, v.av, v.ad, acc);
    }

    // CPU order (ggml_vec_dot_iq4_xs_q8_K, AVX2): eight int32 lanes per superblock, lane l = sum over
    // the eight sub-blocks ib of (ls_ib - 32) * sum_{e = 4l..4l+3} v[32 ib + e] a[32 ib + e], then
    // acc[l] = fma(fp16(x.d) * y.d, (float) sumi[l], acc[l]) over the superblocks and hsum_float_8.
    // Item u holds the sub-blocks 2u and 2u + 1 whole, i.e. its share of all eight lanes; the four
    // items of the quad add up to the lane totals (below 8 * 4 * 127 * 127 * 32 < 2^24: exact as
    // floats). Entry of superblock sb in the scratch, E words: [0..7] the sums, [12] d (FmtKQ's slot).
    template <int NC>
    __device__ static __forceinline__ void dot_ord(const Regs & r, int item, int slot, const lds_act & a, int64_t K, int ncols,
                                                   uint32_t * scr, int cs, int) {
        const int u = item & 3;
        Dec d;
        decode(d, r, item);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && c >= ncols) break;
            int av[16];
            act16(av, a.qs + c * K, item);
            int v[8];
#pragma unroll
            for (int l = 0; l < 8; l++) {
                v[l] = d.ls0 * mi_dot4(d.lv[l], av[l], 0) + d.ls1 * mi_dot4(d.lv[8 + l], av[8 + l], 0);
                v[l] += mi_dpp<MI_DPP_QP_1032>(0, v[l]);  // the quad's other three items (rows are whole
                v[l] += mi_dpp<MI_DPP_QP_2301>(0, v[l]);  // superblocks: a quad is active as one)
            }
            uint32_t * e = scr + c * cs + (slot >> 2) * E;
            if (u == 0) {
                *(uint4 *) e = make_uint4(__float_as_uint((float) v[0]), __float_as_uint((float) v[1]),
                                          __float_as_uint((float) v[2]), __float_as_uint((float) v[3]));
            } else if (u == 1) {
                *(uint4 *) (e + 4) = make_uint4(__float_as_uint((float) v[4]), __float_as_uint((float) v[5]),
                                                __float_as_uint((float) v[6]), __float_as_uint((float) v[7]));
            } else if (u == 2) {
                e[12] = __float_as_uint(d.dw * a.d[c * (K / 256) + (item >> 2)]);
            }
        }
    }
    __device__ static __forceinline__ void chain(const uint32_t * scr, int l, int n_items, int, float & A, float &) {
        const float * e = (const float *) scr;
        const int nsb = n_items >> 2;
        for (int sb = 0; sb < nsb; sb++, e += E) A = fmaf(e[12], e[l], A);
    }
    static int ord_words(int nitems, int & stride) {
        stride = 0;
        return E * (nitems / 4) + 8;
    }
    __device__ static __forceinline__ float finish(float A, float) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A + __shfl_xor(A, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        return z + __shfl_xor(z, 1, 8);
    }
};

// a format's weight load (FmtQ0R's needs the row length)
template <class F>
__device__ __forceinline__ void fmt_load(typename F::Regs & r, const uint8_t * row, int item, int64_t K) {
    if constexpr (F::KL) F::load(r, row, item, K);
    else F::load(r, row, item);
}

// ------------------------------------------------------------------ the streaming kernel

// IPL = items per lane held in the prefetch ring (further items of long rows are loaded
// in-line); PD = rows in flight ahead of the row being computed.
// norm|rms_norm -> mul(g) -> add(b) of the group's activation columns into LDS (f32), by wave 0
// with each column in registers -- the arithmetic of k_norm (ops.hip) and of the F16 GEMV's
// prologue: certified double means, then every step rounded separately. norm_cols: a column's x,
// g, b in registers (every load unconditional at a clamped index, then a select: a load under a
// lane branch makes the compiler wait for it at the branch's join; absent g / b read x instead).
struct norm_cols {
    static constexpr int kJ = (int) (kMiMmvProMaxK / 64);
    float v[kJ], gv[kJ], bv[kJ];
};

__device__ __forceinline__ void norm_cols_load(const mi_mmv_group & g, const char * X, int c, norm_cols & r) {
    const int lane = threadIdx.x & 63;
    const int64_t K = g.K;
    const float * xc = (const float *) (X + c * g.xcol);
    const float * gp = g.pro.g ? g.pro.g : xc;
    const float * bp = g.pro.b ? g.pro.b : xc;
#pragma unroll
    for (int j = 0; j < norm_cols::kJ; j++) {
        const int64_t k = (int64_t) j * 64 + lane;
        const bool in = k < K;
        const int64_t kc = in ? k : K - 1;
        const float xv = xc[kc], gl = gp[kc], bl = bp[kc];
        r.v[j] = in ? xv : 0.0f;
        r.gv[j] = in && g.pro.g ? gl : 1.0f;
        r.bv[j] = in && g.pro.b ? bl : 0.0f;
    }
}

// r: column 0, already loaded (before the weight stream, so that vmcnt does not make it wait for
// the weights); the other columns are loaded here
__device__ void norm_prologue(const mi_mmv_group & g, const char * X, int ncols, float * xn, norm_cols & r) {
    constexpr int kJ = norm_cols::kJ;
    const int lane = threadIdx.x & 63;
    const int64_t K = g.K;
    for (int c = 0; c < ncols; c++) {
        if (c > 0) norm_cols_load(g, X, c, r);
        float scale;
        if (g.pro.mode == 2) {
            const float mean = wave_mean_cpu_order<true, kJ>(r.v, K);
            scale = 1.0f / sqrtf(add_rn(mean, g.pro.eps));
        } else {
            const float mean = wave_mean_cpu_order<false, kJ>(r.v, K);
#pragma unroll
            for (int j = 0; j < kJ; j++) r.v[j] = sub_rn(r.v[j], mean);
            const float variance = wave_mean_cpu_order<true, kJ>(r.v, K);
            scale = 1.0f / sqrtf(add_rn(variance, g.pro.eps));
        }
#pragma unroll
        for (int j = 0; j < kJ; j++) {
            const int64_t k = (int64_t) j * 64 + lane;
            if (k < K) {
                float y = mul_rn(r.v[j], scale);
                if (g.pro.g) y = mul_rn(y, r.gv[j]);
                if (g.pro.b) y = add_rn(y, r.bv[j]);
                xn[c * K + k] = y;
            }
        }
    }
}

// One column with a Q8_K activation (Q4_K / Q5_K weights), K a multiple of 256 up to
// kMiMmvProMaxK: wave 0 holds the column four consecutive elements per lane (k = 256 j + 4 l + i,
// float4 loads), normalizes it in registers and quantizes each 256-slice straight into the LDS
// activations (quantize_slice: the layout mi_q8K_superblock takes) -- no normalized copy through
// LDS, no second barrier and no re-read (round 6). The arithmetic of norm_prologue element for
// element: certified double mean / variance (wave_mean_cpu_order4), then every step rounded.
struct norm_cols4 {
    static constexpr int kJ = (int) (kMiMmvProMaxK / 256);
    float4 v[kJ], gv[kJ], bv[kJ];
};

__device__ __forceinline__ void norm_cols4_load(const mi_mmv_group & g, const char * X, norm_cols4 & r) {
    const int lane = threadIdx.x & 63;
    const int64_t K = g.K;
    const float * xc = (const float *) X;
    const float * gp = g.pro.g ? g.pro.g : xc;
    const float * bp = g.pro.b ? g.pro.b : xc;
#pragma unroll
    for (int j = 0; j < norm_cols4::kJ; j++) {
        const int64_t k = (int64_t) j * 256 + lane * 4;
        const int64_t kc = k < K ? k : K - 4;  // (unconditional loads at clamped addresses; unused past K)
        r.v[j] = *(const float4 *) (xc + kc);
        r.gv[j] = *(const float4 *) (gp + kc);
        r.bv[j] = *(const float4 *) (bp + kc);
    }
}

// Q8_K of J 256-slices held four consecutive floats per lane (slice j: v[j]), all slices' steps
// interleaved (mi_q8K_superblock's arithmetic per slice: the first element of largest |x| keeps its
// sign, iscale = -127 / max, q = min(127, RNE via the fma bit trick), d = 1 / iscale; zero slices
// d = 0), so the slices' wave reductions and divisions overlap instead of running one after the other
template <int J>
__device__ __forceinline__ void quantize_slices_q8K(const float (&v)[J][4], int nsl, int lane, const lds_act & a, int64_t K) {
    uint32_t ab[J];
    int bi[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        float best = 0.0f;
        int bidx = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float ax = fabsf(v[j][i]);
            if (ax > best) { best = ax; bidx = i; }  // first occurrence within the lane
        }
        ab[j] = __float_as_uint(best);
        bi[j] = bidx;
    }
    uint32_t am[J], key[J];
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = ab[j];
    auto mx = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
    auto mn = [](uint32_t x, uint32_t y) { return x < y ? x : y; };
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_QP_1032>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_QP_2301>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_ROW_MIRROR>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_ROW_BCAST15, 0xA>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) am[j] = mx(am[j], (uint32_t) mi_dpp<MI_DPP_ROW_BCAST31, 0xC>(0, (int) am[j]));
#pragma unroll
    for (int j = 0; j < J; j++) {
        am[j] = (uint32_t) __builtin_amdgcn_readlane((int) am[j], 63);
        key[j] = ab[j] == am[j] ? (uint32_t) (lane * 4 + bi[j]) : 0xFFFFFFFFu;
    }
    constexpr int kId = -1;
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_QP_1032>(kId, (int) key[j]));
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_QP_2301>(kId, (int) key[j]));
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_ROW_HALF_MIRROR>(kId, (int) key[j]));
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_ROW_MIRROR>(kId, (int) key[j]));
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_ROW_BCAST15, 0xA>(kId, (int) key[j]));
#pragma unroll
    for (int j = 0; j < J; j++) key[j] = mn(key[j], (uint32_t) mi_dpp<MI_DPP_ROW_BCAST31, 0xC>(kId, (int) key[j]));
    float iscale[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint32_t idx = (uint32_t) __builtin_amdgcn_readlane((int) key[j], 63);
        const int owner = (int) (idx >> 2), sel = (int) (idx & 3);
        const float mine = sel == 0 ? v[j][0] : sel == 1 ? v[j][1] : sel == 2 ? v[j][2] : v[j][3];
        const float vmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), owner & 63));
        iscale[j] = am[j] != 0 ? -127.f / vmax : 0.0f;
    }
    int s[J];
    uint32_t packed[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        packed[j] = 0;
        s[j] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float t = __builtin_fmaf(iscale[j], v[j][i], 12582912.f);
            int q = (__float_as_int(t) & 0x007fffff) - 0x00400000;
            q = q < 127 ? q : 127;
            if (am[j] == 0) q = 0;
            s[j] += q;
            packed[j] |= ((uint32_t) (q & 0xFF)) << (8 * i);
        }
    }
#pragma unroll
    for (int j = 0; j < J; j++) s[j] = mi_sum8(s[j]);
#pragma unroll
    for (int j = 0; j < J; j++) {
        if (j >= nsl) break;  // wave-uniform
        *(uint32_t *) (a.qs + j * 256 + lane * 4) = packed[j];
        if ((lane & 7) == 0) a.s32[j * 8 + (lane >> 3)] = (int16_t) s[j];
        if (lane == 0) a.d[j] = am[j] != 0 ? 1.0f / iscale[j] : 0.0f;
    }
}

__device__ void norm_quant_prologue1(const mi_mmv_group & g, norm_cols4 & r, const lds_act & act) {
    constexpr int kJ = norm_cols4::kJ;
    const int lane = threadIdx.x & 63;
    const int64_t K = g.K;
    const int nsl = (int) (K / 256);
    float scale;
    if (g.pro.mode == 2) {
        const float mean = wave_mean_cpu_order4<true, kJ>(r.v, K);
        scale = 1.0f / sqrtf(add_rn(mean, g.pro.eps));
    } else {
        const float mean = wave_mean_cpu_order4<false, kJ>(r.v, K);
#pragma unroll
        for (int j = 0; j < kJ; j++) {
            r.v[j].x = sub_rn(r.v[j].x, mean);
            r.v[j].y = sub_rn(r.v[j].y, mean);
            r.v[j].z = sub_rn(r.v[j].z, mean);
            r.v[j].w = sub_rn(r.v[j].w, mean);
        }
        const float variance = wave_mean_cpu_order4<true, kJ>(r.v, K);
        scale = 1.0f / sqrtf(add_rn(variance, g.pro.eps));
    }
    float y[kJ][4];
#pragma unroll
    for (int j = 0; j < kJ; j++) {
        const float e[4] = {r.v[j].x, r.v[j].y, r.v[j].z, r.v[j].w};
        const float ge[4] = {r.gv[j].x, r.gv[j].y, r.gv[j].z, r.gv[j].w};
        const float be[4] = {r.bv[j].x, r.bv[j].y, r.bv[j].z, r.bv[j].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float t = mul_rn(e[i], scale);
            if (g.pro.g) t = mul_rn(t, ge[i]);
            if (g.pro.b) t = add_rn(t, be[i]);
            y[j][i] = j < nsl ? t : 0.0f;  // (slices past K: zero, not stored)
        }
    }
    quantize_slices_q8K<kJ>(y, nsl, lane, act, K);
}

// one output element, through the graph's epilogue: + bias[row], then + resid or GELU (the fp16
// table lookup of ggml_vec_gelu_f32 with its +-10 clamps), then the K/V-cache row copies -- each
// step rounded as its own node would round it
// The epilogue operands of a wave's first row, requested in the prologue (a load at store time adds
// a dependent memory round trip at the end of the kernel -- at GPT-2's sizes one row per wave)
template <int NC>
struct epi_pre {
    int row = -1;
    float bias = 0.0f;
    float res[NC];
};
template <int NC>
__device__ __forceinline__ void epi_prefetch(const mi_mmv_group & g, int row, const char * any, epi_pre<NC> & p) {
    const mi_mmv_group::epilogue & e = g.epi;
    p.row = row;
    // unconditional loads at valid addresses (an absent operand reads `any`; its value is unused)
    p.bias = *(e.bias ? e.bias + row : (const float *) any);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int cc = c < g.ncols ? c : g.ncols - 1;
        p.res[c] = *(const float *) (e.resid ? e.resid + cc * e.resid_nb1 + (size_t) row * sizeof(float) : any);
    }
}

template <bool X, int NC = 1>
__device__ __forceinline__ void store_out(const mi_mmv_group & g, float * dst, int c, int row, float v, const epi_pre<NC> * pre = nullptr) {
    if constexpr (!X) {
        *(float *) ((char *) dst + c * g.ycol + (size_t) row * sizeof(float)) = v;
        return;
    }
    const mi_mmv_group::epilogue & e = g.epi;
    const bool hit = pre && row == pre->row;
    float pr = pre ? pre->res[0] : 0.0f;
    if (pre) {
#pragma unroll
        for (int cc = 1; cc < NC; cc++)
            if (c == cc) pr = pre->res[cc];
    }
    if (e.bias) v = v + (hit ? pre->bias : e.bias[row]);
    if (e.resid) v = v + (hit ? pr : *(const float *) (e.resid + c * e.resid_nb1 + (size_t) row * sizeof(float)));
    else if (e.gelu_table) v = v <= -10.0f ? 0.0f : (v >= 10.0f ? v : mi_h2f(e.gelu_table[mi_f2h(v)]));
    *(float *) ((char *) dst + c * g.ycol + (size_t) row * sizeof(float)) = v;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (e.copy[k].ptr && row >= e.copy[k].row0 && row < e.copy[k].row1) {
            *(float *) (e.copy[k].ptr + c * e.copy[k].col_stride + (size_t) (row - e.copy[k].row0) * sizeof(float)) = v;
        }
    }
}

// ORD: combine in the reference CPU's order (bit-identical results, see dot_ord / chain): each
// 64-item chunk of a row leaves its per-item lane sums in the wave's LDS scratch, then lane
// (column c, CPU lane l) runs the reference's sequential fma chain over the chunk.
// PRO: the graph's norm prologue (g.pro) and store epilogue (g.epi) are compiled in
// MR > 1 (one column, rows of at most 16 items: tall short-K matrices such as GPT-2's lm_head,
// K = 768 = 12 Q4_K items): each wave step covers MR rows, 16 lanes per row (lane 16 r + i: item i
// of the step's row r) instead of one row on 64 lanes of which K / ITEM do work
// IDS (GGML_OP_MUL_MAT_ID decode): the member's W field points at its expert id in device memory;
// the workgroup reads it at entry and streams expert id's matrix of the stack g.ids_w (stride
// g.ids_nb02). An id outside [0, g.ids_n_as) ends the workgroup here, before any barrier.
template <class F, int NC, int PD, int IPL, bool TAIL, bool ORD, bool PRO, int MR = 1, bool IDS = false>
__global__ __launch_bounds__(256) void k_mmv_stream(mi_mmv_group g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int NB = PD + 1;  // ring slots
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int member = blockIdx.x / g.blocks_per_member;
    const int rb = blockIdx.x - member * g.blocks_per_member;
    const uint8_t * W = (const uint8_t *) g.m[member].W;
    if constexpr (IDS) {
        const int expert = __builtin_amdgcn_readfirstlane(*(const int32_t *) W);
        if ((unsigned) expert >= (unsigned) g.ids_n_as) return;
        W = (const uint8_t *) g.ids_w + (size_t) expert * g.ids_nb02;
    }
    const char * X = g.m[member].X;
    float * dst = g.m[member].dst;
    const int64_t K = g.K;
    const int nitems = (int) (K / F::ITEM);
    const int ncols = g.ncols;
    const lds_act act = lds_carve<F::QKA>(lds, NC, K);
    uint32_t * scr = (uint32_t *) (lds + ord_offset(lds_bytes<F::QKA>(NC, K))) + wave * (g.ord_rows ? g.ord_rows : 1) * NC * g.ord_cs;

    // 32-bit row bookkeeping (N < 2^31): scalar compares, no 64-bit VGPR temporaries in the loop
    const int Nr = (int) g.N;
    const int row_begin = rb * (int) g.rows_per_block;
    const int row_end = row_begin + (int) g.rows_per_block < Nr ? row_begin + (int) g.rows_per_block : Nr;
    const int nrows = row_end - row_begin > wave ? (row_end - row_begin - wave + 3) / 4 : 0;
    auto wrow_of = [&](int k) {
        const int r = row_begin + 4 * k + wave;
        return W + (size_t) (r < Nr ? r : Nr - 1) * g.nb01;
    };

    // Every load of the ring is unconditional, with clamped row / item indices: a load under a
    // branch makes the compiler merge the ring registers after it, and the merge copy waits for
    // the load just issued (vmcnt(0)), which serialises the prefetch.
    typename F::Regs ring[NB][IPL];
    auto prefetch = [&](typename F::Regs (&slot)[IPL], int k) {
        const uint8_t * wr = wrow_of(k);
#pragma unroll
        for (int i = 0; i < IPL; i++) {
            const int item = lane + 64 * i;
            fmt_load<F>(slot[i], wr, item < nitems ? item : nitems - 1, K);
        }
    };
    // MR > 1: ring slot = one step of MR rows; lane 16 r + i loads item i of row MR k + r
    auto prefetch_mr = [&](typename F::Regs (&slot)[IPL], int k) {
        const uint8_t * wr = wrow_of(MR * k + (lane >> 4));
        const int item = lane & 15;
        fmt_load<F>(slot[0], wr, item < nitems ? item : nitems - 1, K);
    };
    const int nsteps = MR > 1 ? (nrows + MR - 1) / MR : nrows;
    const int klast = nsteps > 0 ? nsteps - 1 : 0;

    // 0) what the prologue reads first, requested before the weights (vmcnt retires in order: a
    //    use of it would otherwise wait for the weight loads too): the norm prologue's first
    //    column, g and b (wave 0), or the activation slices of the first quantization round
    norm_cols nc0;
    // one Q8_K column: normalized and quantized in wave 0's registers (norm_quant_prologue1)
    constexpr bool P4 = PRO && NC == 1 && F::QKA == 256;
    norm_cols4 nc4;
    const bool p4 = P4 && g.pro.mode && g.pro_q;
    const int nsl = (int) (K / 256);
    const int total = nsl * ncols;
    float4 x0[4];  // the first quantization round's slices
    // Q8_K (R16): a round of a wave = slices p0 .. p0 + 3, one per 16-lane row (lane: 16 consecutive
    // elements, quantize_row16); Q8_0: slices p0, p0 + 4, p0 + 8, p0 + 12, four elements per lane
    constexpr bool R16 = F::QKA == 256;
    const int p_first = R16 ? 4 * wave : wave;
    auto load_round = [&](float4 (&v)[4], const char * Xs, size_t xcs, int p0) {
        // unconditional (clamped) loads: a predicated load makes hipcc wait vmcnt(0) per load
        if constexpr (R16) {
            const int p = min(p0 + (lane >> 4), total - 1);
            const int c = p / nsl, sl = p - c * nsl;
            const float4 * src = (const float4 *) (Xs + c * xcs + ((size_t) sl * 256 + (lane & 15) * 16) * sizeof(float));
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = src[u];
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int p = min(p0 + 4 * u, total - 1);
                const int c = p / nsl, sl = p - c * nsl;
                v[u] = *(const float4 *) (Xs + c * xcs + ((size_t) sl * 256 + lane * 4) * sizeof(float));
            }
        }
    };
    epi_pre<NC> epre;
    if constexpr (PRO) {
        // wave 0 alone requests the norm's column. (The load under this branch is waited for at
        // its join, before wave 0 requests its weights; every wave loading the column instead --
        // unconditional, ahead of the weights -- queued waves 1-3's weights behind it: Q4_K GPT-2
        // decode 0.417 -> 0.443 ms/token, profiles/r05t_bench_quick.json)
        if (g.pro.mode && wave == 0) {
            if (p4) norm_cols4_load(g, X, nc4);
            else norm_cols_load(g, X, 0, nc0);
        }
        epi_prefetch<NC>(g, row_begin + wave < Nr ? row_begin + wave : Nr - 1, X, epre);
    } else {
        load_round(x0, X, g.xcol, p_first);
    }
    // (keep these loads ahead of the weight prefetch: the scheduler hoisted the prefetch above
    // them, and vmcnt retires in order -- the activations then waited for the weights)
#ifndef MI_AB_NO_ACT_ORDER  // (A/B builds only)
    asm volatile("" ::: "memory");
#endif
    // 1) the first PD rows' weights in flight
#pragma unroll
    for (int u = 0; u < PD; u++) {
        if constexpr (MR > 1) prefetch_mr(ring[u], u < klast ? u : klast);
        else prefetch(ring[u], u < klast ? u : klast);
    }

    // 2) quantize the member's activation columns into LDS (wave w: 256-slices w, w+4, ...),
    //    from the normalized columns when the graph's norm chain is fused in
    const char * Xq = X;
    size_t xcolq = g.xcol;
    if (PRO && g.pro.mode && p4) {
        // (the activations complete in LDS once wave 0 is through: the barrier below publishes them)
        if (wave == 0) norm_quant_prologue1(g, nc4, act);
    } else if (PRO && g.pro.mode) {
        float * xn = (float *) (lds + g.pro_off);
        if (wave == 0) norm_prologue(g, X, ncols, xn, nc0);
        __syncthreads();
        Xq = (const char *) xn;
        xcolq = (size_t) K * sizeof(float);
    }
    if (!p4) {
        for (int p0 = p_first; p0 < total; p0 += 16) {
            float4 v[4];
            if (!PRO && p0 == p_first) {
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = x0[u];
            } else {
                load_round(v, Xq, xcolq, p0);
            }
            if constexpr (R16) {
                const int p = min(p0 + (lane >> 4), total - 1);
                const int c = p / nsl, sl = p - c * nsl;
                quantize_row16(v, lane, act, K, c, sl, p0 + (lane >> 4) < total);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int p = p0 + 4 * u;
                    if (p < total) {
                        const int c = p / nsl, sl = p - c * nsl;
                        quantize_slice<F::QKA, fmt_s1<F>::value>(v[u], lane, act, K, c, sl);
                    }
                }
            }
        }
    }
    __syncthreads();

    if constexpr (MR > 1) {
        static_assert(NC == 1 && IPL == 1 && !TAIL, "multi-row steps: one column, one item per lane");
        const int rr = lane >> 4, it = lane & 15;
        auto sync = [] {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        };
        for (int k0 = 0; k0 < nsteps; k0 += NB) {
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int k = k0 + u;
                if (k >= nsteps) break;  // wave-uniform
                prefetch_mr(ring[(u + PD) % NB], k + PD < klast ? k + PD : klast);
                const int j = MR * k + rr;  // this lane's row of the wave
                if constexpr (ORD) {
                    // R = g.ord_rows rows (a multiple of MR) collect their lane sums, then one
                    // chain pass: lane 8 r + l runs CPU lane l of row slot r (as the one-row form)
                    const int RS = g.ord_rows / MR, cs = g.ord_cs, S = g.ord_s;
                    const int slot = k % RS;
                    if (it < nitems) F::template dot_ord<1>(ring[u][0], it, it, act, K, ncols, scr + (slot * MR + rr) * cs, cs, S);
                    if (slot == RS - 1 || k == nsteps - 1) {  // wave-uniform
                        sync();
                        const int r = lane >> 3, ll = lane & 7;
                        const int jr = (k - slot) * MR + r;
                        const bool mine = r < (slot + 1) * MR && jr < nrows;
                        float A = 0.0f, M = 0.0f;
                        if (mine) F::chain(scr + r * cs, ll, nitems, S, A, M);
                        const float v = F::finish(A, M);
                        if (ll == 0 && mine) store_out<PRO, 1>(g, dst, 0, row_begin + 4 * jr + wave, v, &epre);
                        sync();
                    }
                } else {
                    float acc[1] = {0.0f};
                    if (it < nitems) F::template dot<1>(ring[u][0], it, act, K, ncols, acc);
                    // sum over the row's 16 lanes (DPP within a 16-lane row)
                    auto f = [](int x) { return __int_as_float(x); };
                    auto i = [](float x) { return __float_as_int(x); };
                    float v = acc[0];
                    v += f(mi_dpp<MI_DPP_QP_1032>(0, i(v)));
                    v += f(mi_dpp<MI_DPP_QP_2301>(0, i(v)));
                    v += f(mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, i(v)));
                    v += f(mi_dpp<MI_DPP_ROW_MIRROR>(0, i(v)));
                    if (it == 0 && j < nrows) store_out<PRO, 1>(g, dst, 0, row_begin + 4 * j + wave, v, &epre);
                }
            }
        }
    } else {
    // (one column, tree order: the lane's items are the same in every row, so their activation
    // operands are read from LDS once, here, instead of per row)
    constexpr bool AREG = NC == 1 && !ORD && !TAIL;
    typename F::Act areg[AREG ? IPL : 1];
    if constexpr (AREG) {
#pragma unroll
        for (int i = 0; i < IPL; i++) {
            const int item = lane + 64 * i;
            F::act_load(areg[i], item < nitems ? item : nitems - 1, act, K);
        }
    }
    // 3) stream: ring slot u holds row k0+u; refill it with row k0+u+PD right before using it
    //    (the last row again past the end: an L2 hit)
    for (int k0 = 0; k0 < nrows; k0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; u++) {
            const int k = k0 + u;
            if (k >= nrows) break;  // wave-uniform
            prefetch(ring[(u + PD) % NB], k + PD < klast ? k + PD : klast);
            const int row = row_begin + 4 * k + wave;
            if constexpr (ORD) {
                const int R = g.ord_rows, cs = g.ord_cs, S = g.ord_s;
                auto sync = [] {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                };
                if (R == 0) {
                    // rows too long for the scratch: one chain pass per 64-item chunk of the row
                    const int cl = lane >> 3, ll = lane & 7;
                    float A = 0.0f, M = 0.0f;
                    auto chunk_done = [&](int base) {
                        sync();
                        if (cl < ncols) F::chain(scr + cl * cs, ll, min(64, nitems - base), S, A, M);
                        sync();
                    };
#pragma unroll
                    for (int i = 0; i < IPL; i++) {
                        if (64 * i >= nitems) break;  // wave-uniform
                        const int item = lane + 64 * i;
                        if (item < nitems) F::template dot_ord<NC>(ring[u][i], item, lane, act, K, ncols, scr, cs, S);
                        chunk_done(64 * i);
                    }
                    if constexpr (TAIL) {
                        const uint8_t * wr = wrow_of(k);
                        for (int base = 64 * IPL; base < nitems; base += 64) {
                            const int item = base + lane;
                            if (item < nitems) {
                                typename F::Regs rr;
                                fmt_load<F>(rr, wr, item, K);
                                F::template dot_ord<NC>(rr, item, lane, act, K, ncols, scr, cs, S);
                            }
                            chunk_done(base);
                        }
                    }
                    const float v = F::finish(A, M);
                    if (ll == 0 && cl < ncols) store_out<PRO, NC>(g, dst, cl, row, v, &epre);
                    continue;
                }
                // whole rows in the scratch: R rows' lane sums are collected, then one chain pass
                // runs them all, lane = (row r, column c, CPU lane l), 8 * NC * R <= 64
                const int slot = k % R;
                uint32_t * srow = scr + slot * NC * cs;
#pragma unroll
                for (int i = 0; i < IPL; i++) {
                    const int item = lane + 64 * i;
                    if (item < nitems) F::template dot_ord<NC>(ring[u][i], item, item, act, K, ncols, srow, cs, S);
                }
                if constexpr (TAIL) {
                    const uint8_t * wr = wrow_of(k);
                    for (int item = lane + 64 * IPL; item < nitems; item += 64) {
                        typename F::Regs rr;
                        fmt_load<F>(rr, wr, item, K);
                        F::template dot_ord<NC>(rr, item, item, act, K, ncols, srow, cs, S);
                    }
                }
                if (slot == R - 1 || k == nrows - 1) {  // wave-uniform
                    sync();
                    const int r = lane / (8 * NC), cl = (lane >> 3) % NC, ll = lane & 7;
                    const bool mine = r <= slot && cl < ncols;
                    float A = 0.0f, M = 0.0f;
                    if (mine) F::chain(scr + (r * NC + cl) * cs, ll, nitems, S, A, M);
                    const float v = F::finish(A, M);
                    if (ll == 0 && mine) {
                        store_out<PRO, NC>(g, dst, cl, row_begin + 4 * (k - slot + r) + wave, v, &epre);
                    }
                    sync();
                }
                continue;
            }
            float acc[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] = 0.0f;
#pragma unroll
            for (int i = 0; i < IPL; i++) {
                const int item = lane + 64 * i;
                if constexpr (AREG) {
                    if (item < nitems) acc[0] = F::dot_act(ring[u][i], item, areg[i], acc[0]);
                } else {
                    if (item < nitems) F::template dot<NC>(ring[u][i], item, act, K, ncols, acc);
                }
            }
            if constexpr (TAIL) {
                // items beyond the ring's IPL per lane, loaded in-line (long rows only: a loop
                // with loads here makes the compiler drain vmcnt at the top of every row group)
                const uint8_t * wr = wrow_of(k);
                for (int item = lane + 64 * IPL; item < nitems; item += 64) {
                    typename F::Regs rr;
                    fmt_load<F>(rr, wr, item, K);
                    F::template dot<NC>(rr, item, act, K, ncols, acc);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float v = mi_wave_sum_u(acc[c]);
                if (lane == 0 && c < ncols) store_out<PRO, NC>(g, dst, c, row, v, &epre);
            }
        }
    }
    }
}

// Workgroups that fit on the chip at once for this kernel instance (all of them are launched
// in one wave, so no workgroup waits for another to retire). Speed only: nothing relies on
// co-residency. Cached per kernel.
int resident_blocks(const void * fn, size_t lds) {
    struct entry { const void * fn; size_t lds; int n; };
    static entry cache[64];
    static int ncache = 0;
    for (int i = 0; i < ncache; i++) if (cache[i].fn == fn && cache[i].lds == lds) return cache[i].n;
    int dev = 0, per_cu = 0;
    hipDeviceProp_t prop;
    (void) hipGetDevice(&dev);
    (void) hipGetDeviceProperties(&prop, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int n = per_cu * prop.multiProcessorCount;
    if (ncache < 64) cache[ncache++] = entry{fn, lds, n};
    return n;
}

static int mi_cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        (void) hipGetDevice(&dev);
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return n;
}

// The route string of one k_mmv_stream instance (g_mi_last_route), built once per instance: the weight
// format (the ggml type number unless the format reads pairs of blocks or a repacked copy) and the
// template arguments that tell the instances apart.
template <class F, int NC, int PD, int IPL, bool TAIL, bool ORD, bool PRO, int MR, bool IDS>
const char * stream_route(int type) {
    static char name[96] = "";
    if (!name[0]) {
        const char * fmt = std::is_same<F, FmtQ0Pair>::value ? "pairs," : std::is_same<F, FmtQ0R>::value || std::is_same<F, FmtQ8R>::value ? "repacked," : "";
        snprintf(name, sizeof(name), "k_mmv_stream<type%d,%snc%d,pd%d,ipl%d,tail%d,ord%d,pro%d,mr%d,ids%d>", type, fmt, NC, PD, IPL,
                 (int) TAIL, (int) ORD, (int) PRO, MR, (int) IDS);
    }
    return name;
}

template <class F, int NC, int PD, int IPL, bool TAIL, bool ORD, bool PRO = false, int MR = 1, bool IDS = false>
void launch_one(mi_mmv_group g, hipStream_t s) {
    const size_t act = lds_bytes<F::QKA>(NC, g.K);
    size_t lds = act;
    if constexpr (ORD) {
        // whole rows in the scratch when R >= 1 rows per wave fit a 36 KB budget (the kernel is
        // VGPR-limited to ~4 workgroups per CU anyway), else one chunk of 64 items per wave
        const int nitems = (int) (g.K / F::ITEM);
        int S = 0;
        const int cs = F::ord_words(nitems, S);
        int R = (int) ((36 * 1024) / ((size_t) 4 * NC * cs * 4));
        if (R > 8 / NC) R = 8 / NC;
        if (MR > 1) R = R >= MR ? R / MR * MR : 0;  // whole multi-row steps per chain pass (0: refused below)
        if (R >= 1) {
            g.ord_rows = R;
            g.ord_cs = cs;
            g.ord_s = S;
        } else {
            g.ord_rows = 0;
            g.ord_cs = F::ord_words(64, S);
            g.ord_s = S;
        }
        lds = ord_offset(act) + (size_t) 4 * (g.ord_rows ? g.ord_rows : 1) * NC * g.ord_cs * 4;
    }
    if constexpr (MR > 1 && ORD) {
        if (g.ord_rows < MR) {  // a chain pass must hold whole multi-row steps: the one-row form
            launch_one<F, NC, PD, IPL, TAIL, ORD, PRO, 1, IDS>(g, s);
            return;
        }
    }
    g.pro_q = PRO && NC == 1 && F::QKA == 256 && g_mi_tuning.mmv_pro4 ? 1 : 0;
    if (PRO && g.pro.mode) {
        g.pro_off = (int) ord_offset(lds);
        lds = (size_t) g.pro_off + (size_t) NC * g.K * sizeof(float);
    }
    const void * fn = (const void *) k_mmv_stream<F, NC, PD, IPL, TAIL, ORD, PRO, MR, IDS>;
    if (lds > 64 * 1024) {
        static bool attr_set = false;  // per instance
        if (!attr_set) {
            (void) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr_set = true;
        }
    }
    // automatic grid: the resident workgroup count, split over the members. A lone member at
    // K >= 4096 gets one workgroup per CU instead: every workgroup quantizes the whole activation
    // in its prologue, so at 4 rows per workgroup that redundant work dominates (Q4_K 4096^2 alone
    // in its graph 7.96 -> 6.57 us, profiles/r04e_pf_single_blocks.txt)
    int target = g_mi_tuning.mmv_blocks > 0 ? g_mi_tuning.mmv_blocks : resident_blocks(fn, lds);
    if (g_mi_tuning.mmv_blocks <= 0 && g.n == 1 && g.K >= 4096) target = std::min(target, mi_cu_count());
    // Q5_K grouped launches: twice the resident count (smaller workgroups, a later tail; 4096 x 11008
    // 5.56 -> 5.75 TB/s, r04r_gemv_sweep.txt)
    // Q4_K tall members (4096 x 11008): the same (5.47-5.49 -> 5.56-5.62 TB/s on one box,
    // profiles/r05sw_gemv_blocks_sweep.txt; 4096^2 members unchanged within noise, left alone)
    else if (g_mi_tuning.mmv_blocks <= 0 && !ORD && !PRO &&
             (std::is_same<F, FmtKQ<true>>::value || (std::is_same<F, FmtKQ<false>>::value && g.N >= 8192))) target *= 2;
    int bpm = target / g.n;
    if (bpm < 1) bpm = 1;
    int64_t rows = (g.N + bpm - 1) / bpm;
    rows = (rows + 3) / 4 * 4;
    g.rows_per_block = rows;
    g.blocks_per_member = (int) ((g.N + rows - 1) / rows);
    mi_route(stream_route<F, NC, PD, IPL, TAIL, ORD, PRO, MR, IDS>(g.type));
    hipLaunchKernelGGL((k_mmv_stream<F, NC, PD, IPL, TAIL, ORD, PRO, MR, IDS>), dim3((unsigned) (g.blocks_per_member * g.n)), dim3(256), lds,
                       s, g);
}


template <class F, int NC, int PD, int IPL, bool ORD>
void launch_tail(const mi_mmv_group & g, hipStream_t s) {
    if (g.K / F::ITEM > 64 * IPL) launch_one<F, NC, PD, IPL, true, ORD>(g, s);
    else launch_one<F, NC, PD, IPL, false, ORD>(g, s);
}

// formats that read the canonical blocks (MUL_MAT_ID has no repacked copies: those need 2-D leaves)
template <class F> constexpr bool kFmtCanonical = !std::is_same<F, FmtQ0R>::value && !std::is_same<F, FmtQ8R>::value;

template <class F, int NC, bool ORD>
void launch_stream(const mi_mmv_group & g, int variant, hipStream_t s) {
    const int items = (int) (g.K / F::ITEM);
    const mi_mmv_group::epilogue & e = g.epi;
    // (Instances that waited for a lone member's activation loads before requesting any weight measured
    // 5.45 us per graph against 4.95 us without the wait: removed)
    const bool pro_epi = g.pro.mode || e.bias || e.resid || e.gelu_table || e.copy[0].ptr || e.copy[1].ptr;
    if constexpr (NC == 1 && kFmtCanonical<F>) {
        // MUL_MAT_ID decode: the plain one-column forms with the device-resolved weight base
        // (no prologue / epilogue, no repacked copies)
        if (g.ids_w) {
            if (items > 128) launch_one<F, 1, 2, 2, true, ORD, false, 1, true>(g, s);
            else if (items > 64) launch_one<F, 1, 2, 2, false, ORD, false, 1, true>(g, s);
            else if (variant / 10 == 1) launch_one<F, 1, 1, 1, false, ORD, false, 1, true>(g, s);
            else if (variant / 10 == 3) launch_one<F, 1, 3, 1, false, ORD, false, 1, true>(g, s);
            else launch_one<F, 1, 2, 1, false, ORD, false, 1, true>(g, s);
            return;
        }
    }
    if constexpr (NC == 1) {
        // tall lone members with rows of <= 16 items (GPT-2 lm_head: 50257 x 768, 12 Q4_K items per
        // row): four rows per wave step on 16 lanes each (MR = 4); variant 9x: the one-row form
        if (g.n == 1 && g.N >= 16384 && items <= 16 && variant / 10 != 9) {
            if (pro_epi) launch_one<F, 1, 4, 1, false, ORD, true, 4>(g, s);
            else launch_one<F, 1, 4, 1, false, ORD, false, 4>(g, s);
            return;
        }
    }
    if (pro_epi) {
        // the graph's norm prologue and/or epilogue: instances of their own (prefetch depth 1) so
        // that their registers and per-row branches do not weigh on the plain kernels
        if (items > 128) launch_one<F, NC, 1, 2, true, ORD, true>(g, s);
        else if (items > 64) launch_one<F, NC, 1, 2, false, ORD, true>(g, s);
        else launch_one<F, NC, 1, 1, false, ORD, true>(g, s);
        return;
    }
    if (items > 64) {
        // two items per lane in the ring (Q4_0 / Q8_0 at K=4096)
        if (variant / 10 == 1) launch_tail<F, NC, 1, 2, ORD>(g, s);
        else launch_tail<F, NC, 2, 2, ORD>(g, s);
        return;
    }
    switch (variant / 10) {
        case 1: launch_one<F, NC, 1, 1, false, ORD>(g, s); break;
        case 3: launch_one<F, NC, 3, 1, false, ORD>(g, s); break;
        default: launch_one<F, NC, 2, 1, false, ORD>(g, s); break;
    }
}

template <class F, bool ORD>
void launch_stream_nc(const mi_mmv_group & g, int variant, hipStream_t s) {
    switch (g.ncols) {
        case 1: launch_stream<F, 1, ORD>(g, variant, s); break;
        case 2: launch_stream<F, 2, ORD>(g, variant, s); break;
        case 3: case 4: launch_stream<F, 4, ORD>(g, variant, s); break;
        default: launch_stream<F, 8, ORD>(g, variant, s); break;
    }
}

template <class F>
void launch_stream_ord(const mi_mmv_group & g, int variant, hipStream_t s) {
    if (mi_mmv_order()) launch_stream_nc<F, true>(g, variant, s);
    else launch_stream_nc<F, false>(g, variant, s);
}


} // namespace
