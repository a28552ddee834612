// ggml_quants_host.cpp -- ggml_quantize_chunk (include/ggml/ggml.h:2240-2254) for the weight
// formats on the hot path: Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS
// (+ F16 / F32 passthrough).
//
// These produce the bytes the MI355X kernels consume. They must be bit-identical to the
// reference's imatrix == NULL path (src/ggml.c:21594-21660 -> src/ggml-quants.c reference
// quantizers), which its x86 build compiles with -mfma and gcc's default FP contraction.
// This file is compiled with the same flags and keeps the reference's expression shapes
// where the rounding depends on them; tests/test_core.py checks it against the golden vectors.

#include "ggml_abi.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int kQK4_0 = 32;
constexpr int kQK8_0 = 32;
constexpr int kQKK = 256;

struct blk_q4_0 { ggml_fp16_t d; uint8_t qs[16]; };
struct blk_q8_0 { ggml_fp16_t d; int8_t qs[32]; };
struct blk_q4_K { ggml_fp16_t d, dmin; uint8_t scales[12]; uint8_t qs[128]; };
struct blk_q5_K { ggml_fp16_t d, dmin; uint8_t scales[12]; uint8_t qh[32]; uint8_t qs[128]; };
struct blk_q6_K { uint8_t ql[128]; uint8_t qh[64]; int8_t scales[16]; ggml_fp16_t d; };
static_assert(sizeof(blk_q4_0) == 18 && sizeof(blk_q8_0) == 34 && sizeof(blk_q4_K) == 144 && sizeof(blk_q5_K) == 176, "blocks");
static_assert(sizeof(blk_q6_K) == 210, "blocks");
struct blk_q2_K { uint8_t scales[16]; uint8_t qs[64]; ggml_fp16_t d, dmin; };
struct blk_q3_K { uint8_t hmask[32]; uint8_t qs[64]; uint8_t scales[12]; ggml_fp16_t d; };
static_assert(sizeof(blk_q2_K) == 84 && sizeof(blk_q3_K) == 110, "blocks");
struct blk_iq4_nl { ggml_fp16_t d; uint8_t qs[16]; };
struct blk_iq4_xs { ggml_fp16_t d; uint16_t scales_h; uint8_t scales_l[4]; uint8_t qs[128]; };
static_assert(sizeof(blk_iq4_nl) == 18 && sizeof(blk_iq4_xs) == 136, "blocks");
struct blk_q4_1 { ggml_fp16_t d, m; uint8_t qs[16]; };
struct blk_q5_0 { ggml_fp16_t d; uint8_t qh[4]; uint8_t qs[16]; };
struct blk_q5_1 { ggml_fp16_t d, m; uint8_t qh[4]; uint8_t qs[16]; };
static_assert(sizeof(blk_q4_1) == 20 && sizeof(blk_q5_0) == 22 && sizeof(blk_q5_1) == 24, "blocks");

// src/ggml-quants.c:1097-1102: round half to even through the 1.5*2^23 bias
inline int rne_int(float v) {
    float t = v + 12582912.f;
    int32_t bits;
    memcpy(&bits, &t, 4);
    return (bits & 0x007fffff) - 0x00400000;
}

template <typename T> inline T clampv(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

// src/ggml-quants.c:260-295
void quantize_q4_0_rows(const float * x, blk_q4_0 * y, int64_t n) {
    for (int64_t b = 0; b < n / kQK4_0; ++b, x += kQK4_0) {
        float amax = 0.0f, extreme = 0.0f;
        for (int j = 0; j < kQK4_0; ++j) {
            if (amax < fabsf(x[j])) {
                amax = fabsf(x[j]);
                extreme = x[j];
            }
        }
        const float d = extreme / -8;
        const float id = d ? 1.0f / d : 0.0f;
        y[b].d = ggml_fp32_to_fp16(d);
        for (int j = 0; j < kQK4_0 / 2; ++j) {
            const float v0 = x[j] * id;
            const float v1 = x[kQK4_0 / 2 + j] * id;
            const int q0 = std::min(15, (int) (int8_t) (v0 + 8.5f));
            const int q1 = std::min(15, (int) (int8_t) (v1 + 8.5f));
            y[b].qs[j] = (uint8_t) (q0 | (q1 << 4));
        }
    }
}

// The 32-element min/max and signed-max formats below round a level as (int8_t) (v * id + c). The
// reference's x86 build (gcc -O3 -mfma) contracts that product into the add of the constant, one
// fma, in the scalar and in the vectorised form of the loop alike; it is written out here so that
// the bytes do not depend on this file's compiler (tests/test_legacy_quants.py pins it against
// the reference library).
inline int level_fma(float v, float id, float c) { return (int) (int8_t) fmaf(v, id, c); }

// src/ggml-quants.c:302-337 quantize_row_q4_1_reference: d = (max - min) / 15, m = min,
// q = min(15, (int8_t) ((x - min) * id + 0.5))
void quantize_q4_1_rows(const float * x, blk_q4_1 * y, int64_t n) {
    for (int64_t b = 0; b < n / 32; ++b, x += 32) {
        float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
        for (int j = 0; j < 32; ++j) {
            if (x[j] < lo) lo = x[j];
            if (x[j] > hi) hi = x[j];
        }
        const float d = (hi - lo) / 15;
        const float id = d ? 1.0f / d : 0.0f;
        y[b].d = ggml_fp32_to_fp16(d);
        y[b].m = ggml_fp32_to_fp16(lo);
        for (int j = 0; j < 16; ++j) {
            const int q0 = std::min(15, level_fma(x[j] - lo, id, 0.5f));
            const int q1 = std::min(15, level_fma(x[16 + j] - lo, id, 0.5f));
            y[b].qs[j] = (uint8_t) ((uint8_t) q0 | ((uint8_t) q1 << 4));
        }
    }
}

// src/ggml-quants.c:343-385 quantize_row_q5_0_reference: the first element of largest |x| keeps its
// sign, d = max / -16, q = min(31, (int8_t) (x * id + 16.5)); bit j of qh = the fifth bit of element j
void quantize_q5_0_rows(const float * x, blk_q5_0 * y, int64_t n) {
    for (int64_t b = 0; b < n / 32; ++b, x += 32) {
        float amax = 0.0f, extreme = 0.0f;
        for (int j = 0; j < 32; ++j) {
            if (amax < fabsf(x[j])) {
                amax = fabsf(x[j]);
                extreme = x[j];
            }
        }
        const float d = extreme / -16;
        const float id = d ? 1.0f / d : 0.0f;
        y[b].d = ggml_fp32_to_fp16(d);
        uint32_t qh = 0;
        for (int j = 0; j < 16; ++j) {
            const uint8_t q0 = (uint8_t) std::min(31, level_fma(x[j], id, 16.5f));
            const uint8_t q1 = (uint8_t) std::min(31, level_fma(x[16 + j], id, 16.5f));
            y[b].qs[j] = (uint8_t) ((q0 & 0x0F) | ((q1 & 0x0F) << 4));
            qh |= ((q0 & 0x10u) >> 4) << j;
            qh |= ((q1 & 0x10u) >> 4) << (j + 16);
        }
        memcpy(y[b].qh, &qh, 4);
    }
}

// src/ggml-quants.c:391-433 quantize_row_q5_1_reference: d = (max - min) / 31, m = min,
// q = (uint8_t) ((x - min) * id + 0.5) (no clamp: the fifth bit and the nibble are masked out of it)
void quantize_q5_1_rows(const float * x, blk_q5_1 * y, int64_t n) {
    for (int64_t b = 0; b < n / 32; ++b, x += 32) {
        float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
        for (int j = 0; j < 32; ++j) {
            if (x[j] < lo) lo = x[j];
            if (x[j] > hi) hi = x[j];
        }
        const float d = (hi - lo) / 31;
        const float id = d ? 1.0f / d : 0.0f;
        y[b].d = ggml_fp32_to_fp16(d);
        y[b].m = ggml_fp32_to_fp16(lo);
        uint32_t qh = 0;
        for (int j = 0; j < 16; ++j) {
            const uint8_t q0 = (uint8_t) (int) fmaf(x[j] - lo, id, 0.5f);
            const uint8_t q1 = (uint8_t) (int) fmaf(x[16 + j] - lo, id, 0.5f);
            y[b].qs[j] = (uint8_t) ((q0 & 0x0F) | ((q1 & 0x0F) << 4));
            qh |= ((q0 & 0x10u) >> 4) << j;
            qh |= ((q1 & 0x10u) >> 4) << (j + 16);
        }
        memcpy(y[b].qh, &qh, 4);
    }
}

// src/ggml-quants.c:440-463 (scalar reference; the weight path uses it, :3066-3071)
void quantize_q8_0_rows(const float * x, blk_q8_0 * y, int64_t n) {
    for (int64_t b = 0; b < n / kQK8_0; ++b, x += kQK8_0) {
        float amax = 0.0f;
        for (int j = 0; j < kQK8_0; ++j) amax = std::max(amax, fabsf(x[j]));
        const float d = amax / ((1 << 7) - 1);
        const float id = d ? 1.0f / d : 0.0f;
        y[b].d = ggml_fp32_to_fp16(d);
        for (int j = 0; j < kQK8_0; ++j) y[b].qs[j] = (int8_t) roundf(x[j] * id);
    }
}

// src/ggml-quants.c:1275-1354 make_qkx2_quants: weighted (scale, min) search for one 32-group
float search_scale_min(int nmax, const float * x, const float * w, uint8_t * L, float * out_min,
                       float rmin, float rdelta, int nstep) {
    constexpr int n = 32;
    uint8_t Laux[n];
    float lo = x[0], hi = x[0];
    float sum_w = w[0];
    float sum_x = sum_w * x[0];
    for (int i = 1; i < n; ++i) {
        if (x[i] < lo) lo = x[i];
        if (x[i] > hi) hi = x[i];
        float wi = w[i];
        sum_w += wi;
        sum_x += wi * x[i];
    }
    if (lo > 0) lo = 0;
    if (hi == lo) {
        memset(L, 0, n);
        *out_min = -lo;
        return 0.f;
    }
    float iscale = nmax / (hi - lo);
    float scale = 1 / iscale;
    float best = 0;
    for (int i = 0; i < n; ++i) {
        int l = rne_int(iscale * (x[i] - lo));
        L[i] = (uint8_t) clampv(l, 0, nmax);
        float diff = scale * L[i] + lo - x[i];
        diff = diff * diff;
        float wi = w[i];
        best += wi * diff;
    }
    for (int is = 0; is <= nstep; ++is) {
        iscale = (rmin + rdelta * is + nmax) / (hi - lo);
        float sum_l = 0, sum_l2 = 0, sum_xl = 0;
        for (int i = 0; i < n; ++i) {
            int l = rne_int(iscale * (x[i] - lo));
            l = clampv(l, 0, nmax);
            Laux[i] = (uint8_t) l;
            float wi = w[i];
            sum_l += wi * l;
            sum_l2 += wi * l * l;
            sum_xl += wi * l * x[i];
        }
        float D = sum_w * sum_l2 - sum_l * sum_l;
        if (D > 0) {
            float this_scale = (sum_w * sum_xl - sum_x * sum_l) / D;
            float this_min = (sum_l2 * sum_x - sum_l * sum_xl) / D;
            if (this_min > 0) {
                this_min = 0;
                this_scale = sum_xl / sum_l2;
            }
            float mad = 0;
            for (int i = 0; i < n; ++i) {
                float diff = this_scale * Laux[i] + this_min - x[i];
                diff = diff * diff;
                float wi = w[i];
                mad += wi * diff;
            }
            if (mad < best) {
                memcpy(L, Laux, n);
                best = mad;
                scale = this_scale;
                lo = this_min;
            }
        }
    }
    *out_min = -lo;
    return scale;
}

// src/ggml-quants.c:1357-1364
inline void unpack_scale_min(int j, const uint8_t * q, uint8_t & sc, uint8_t & m) {
    if (j < 4) {
        sc = q[j] & 63;
        m = q[j + 4] & 63;
    } else {
        sc = (uint8_t) ((q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4));
        m = (uint8_t) ((q[j + 4] >> 4) | ((q[j] >> 6) << 4));
    }
}

// Per-superblock scale search + 6-bit packing + final levels, shared by Q4_K (nmax 15) and
// Q5_K (nmax 31): src/ggml-quants.c:2085-2160 / :2339-2390.
template <int NMAX>
void kquant_superblock(const float * x, ggml_fp16_t & d_out, ggml_fp16_t & dmin_out, uint8_t * scales, uint8_t * L) {
    constexpr float rmin = NMAX == 15 ? -1.f : -0.5f;
    constexpr int nstep = NMAX == 15 ? 20 : 15;
    float w[32], mins[8], scl[8];
    float max_scale = 0, max_min = 0;
    for (int j = 0; j < 8; ++j) {
        float sum_x2 = 0;
        for (int l = 0; l < 32; ++l) sum_x2 += x[32 * j + l] * x[32 * j + l];
        float av_x = sqrtf(sum_x2 / 32);
        for (int l = 0; l < 32; ++l) w[l] = av_x + fabsf(x[32 * j + l]);
        scl[j] = search_scale_min(NMAX, x + 32 * j, w, L + 32 * j, &mins[j], rmin, 0.1f, nstep);
        if (scl[j] > max_scale) max_scale = scl[j];
        if (mins[j] > max_min) max_min = mins[j];
    }
    float inv_scale = max_scale > 0 ? 63.f / max_scale : 0.f;
    float inv_min = max_min > 0 ? 63.f / max_min : 0.f;
    memset(scales, 0, 12);
    for (int j = 0; j < 8; ++j) {
        uint8_t ls = (uint8_t) rne_int(inv_scale * scl[j]);
        uint8_t lm = (uint8_t) rne_int(inv_min * mins[j]);
        ls = std::min<uint8_t>(63, ls);
        lm = std::min<uint8_t>(63, lm);
        if (j < 4) {
            scales[j] = ls;
            scales[j + 4] = lm;
        } else {
            scales[j + 4] = (uint8_t) ((ls & 0xF) | ((lm & 0xF) << 4));
            scales[j - 4] |= (uint8_t) ((ls >> 4) << 6);
            scales[j] |= (uint8_t) ((lm >> 4) << 6);
        }
    }
    d_out = ggml_fp32_to_fp16(max_scale / 63.f);
    dmin_out = ggml_fp32_to_fp16(max_min / 63.f);
    for (int j = 0; j < 8; ++j) {
        uint8_t sc, m;
        unpack_scale_min(j, scales, sc, m);
        const float d = ggml_fp16_to_fp32(d_out) * sc;
        if (!d) continue;
        const float dm = ggml_fp16_to_fp32(dmin_out) * m;
        for (int ii = 0; ii < 32; ++ii) {
            int l = rne_int((x[32 * j + ii] + dm) / d);
            L[32 * j + ii] = (uint8_t) clampv(l, 0, NMAX);
        }
    }
}

void quantize_q4_K_rows(const float * x, blk_q4_K * y, int64_t n) {
    uint8_t L[kQKK];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        kquant_superblock<15>(x, y[b].d, y[b].dmin, y[b].scales, L);
        for (int c = 0; c < 4; ++c)
            for (int l = 0; l < 32; ++l) y[b].qs[32 * c + l] = (uint8_t) (L[64 * c + l] | (L[64 * c + 32 + l] << 4));
    }
}

void quantize_q5_K_rows(const float * x, blk_q5_K * y, int64_t n) {
    uint8_t L[kQKK];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        kquant_superblock<31>(x, y[b].d, y[b].dmin, y[b].scales, L);
        memset(y[b].qh, 0, 32);
        for (int c = 0; c < 4; ++c) {
            for (int l = 0; l < 32; ++l) {
                int lo = L[64 * c + l], hi = L[64 * c + 32 + l];
                if (lo > 15) { lo -= 16; y[b].qh[l] |= (uint8_t) (1u << (2 * c)); }
                if (hi > 15) { hi -= 16; y[b].qh[l] |= (uint8_t) (2u << (2 * c)); }
                y[b].qs[32 * c + l] = (uint8_t) (lo | (hi << 4));
            }
        }
    }
}

// nearest_int(a * b) as the reference's -mfma build computes it: the product is contracted into
// the bias add, fma(a, b, 1.5 * 2^23)
inline int rne_int_fma(float a, float b) {
    float t = fmaf(a, b, 12582912.f);
    int32_t bits;
    memcpy(&bits, &t, 4);
    return (bits & 0x007fffff) - 0x00400000;
}

// a product rounded to f32 on its own, which the compiler may not contract into a following add
inline float mul_rn(float a, float b) {
    float r = a * b;
    __asm__("" : "+x"(r));
    return r;
}

// src/ggml-quants.c:1104-1171 make_qx_quants(n = 16, nmax = 32, rmse_type = 1, qw = NULL): the
// symmetric scale of one 16-element sub-block, weights x^2, searched over 19 candidate scales.
// L gets the levels + 32. The roundings are written out as the reference's x86 build
// (make_qx_quants.constprop, gcc -O3 -mfma) performs them, because they differ between its loops:
// the first pass is scalar and contracts sumlx = fma(w*x, l, sumlx), suml2 = fma(w*l, l, suml2);
// the candidate loop is vectorised, so its products (w*x)*l and (w*l)*l are rounded on their own
// and then added in element order; nmax + 0.1f*is is one fma (nmax is a run-time argument there).
float search_scale_sym16(const float * x, int8_t * L) {
    constexpr int n = 16, nmax = 32;
    float max = 0;
    float amax = 0;
    for (int i = 0; i < n; ++i) {
        float ax = fabsf(x[i]);
        if (ax > amax) { amax = ax; max = x[i]; }
    }
    if (amax < 1e-30f) {  // all zero
        for (int i = 0; i < n; ++i) L[i] = 0;
        return 0.f;
    }
    float iscale = -nmax / max;
    float sumlx = 0;
    float suml2 = 0;
    for (int i = 0; i < n; ++i) {
        int l = rne_int_fma(iscale, x[i]);
        l = std::max(-nmax, std::min(nmax - 1, l));
        L[i] = (int8_t) (l + nmax);
        float w = x[i] * x[i];
        sumlx = fmaf(w * x[i], (float) l, sumlx);
        suml2 = fmaf(w * (float) l, (float) l, suml2);
    }
    float scale = sumlx / suml2;
    float best = scale * sumlx;
    for (int is = -9; is <= 9; ++is) {
        if (is == 0) continue;
        iscale = -fmaf(0.1f, (float) is, (float) nmax) / max;
        sumlx = suml2 = 0;
        for (int i = 0; i < n; ++i) {
            int l = rne_int_fma(iscale, x[i]);
            l = std::max(-nmax, std::min(nmax - 1, l));
            float w = x[i] * x[i];
            sumlx += mul_rn(w * x[i], (float) l);
            suml2 += mul_rn(w * (float) l, (float) l);
        }
        if (suml2 > 0 && sumlx * sumlx > best * suml2) {
            for (int i = 0; i < n; ++i) {
                int l = rne_int_fma(iscale, x[i]);
                L[i] = (int8_t) (nmax + std::max(-nmax, std::min(nmax - 1, l)));
            }
            scale = sumlx / suml2;
            best = scale * sumlx;
        }
    }
    return scale;
}

// src/ggml-quants.c:2631-2711 quantize_row_q6_K_reference
void quantize_q6_K_rows(const float * x, blk_q6_K * y, int64_t n) {
    int8_t L[kQKK];
    float scales[kQKK / 16];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        float max_scale = 0;
        float max_abs_scale = 0;
        for (int ib = 0; ib < kQKK / 16; ++ib) {
            const float scale = search_scale_sym16(x + 16 * ib, L + 16 * ib);
            scales[ib] = scale;
            const float abs_scale = fabsf(scale);
            if (abs_scale > max_abs_scale) {
                max_abs_scale = abs_scale;
                max_scale = scale;
            }
        }
        if (!max_abs_scale) {
            memset(&y[b], 0, sizeof(blk_q6_K));
            y[b].d = ggml_fp32_to_fp16(0.f);
            continue;
        }
        float iscale = -128.f / max_scale;
        y[b].d = ggml_fp32_to_fp16(1 / iscale);
        for (int ib = 0; ib < kQKK / 16; ++ib) y[b].scales[ib] = (int8_t) std::min(127, rne_int_fma(iscale, scales[ib]));
        for (int j = 0; j < kQKK / 16; ++j) {
            float d = ggml_fp16_to_fp32(y[b].d) * y[b].scales[j];
            if (!d) continue;
            for (int ii = 0; ii < 16; ++ii) {
                int l = rne_int(x[16 * j + ii] / d);
                l = std::max(-32, std::min(31, l));
                L[16 * j + ii] = (int8_t) (l + 32);
            }
        }
        uint8_t * ql = y[b].ql;
        uint8_t * qh = y[b].qh;
        for (int j = 0; j < kQKK; j += 128) {
            for (int l = 0; l < 32; ++l) {
                const uint8_t q1 = L[j + l + 0] & 0xF;
                const uint8_t q2 = L[j + l + 32] & 0xF;
                const uint8_t q3 = L[j + l + 64] & 0xF;
                const uint8_t q4 = L[j + l + 96] & 0xF;
                ql[l + 0] = (uint8_t) (q1 | (q3 << 4));
                ql[l + 32] = (uint8_t) (q2 | (q4 << 4));
                qh[l] = (uint8_t) ((L[j + l] >> 4) | ((L[j + l + 32] >> 4) << 2) | ((L[j + l + 64] >> 4) << 4) | ((L[j + l + 96] >> 4) << 6));
            }
            ql += 64;
            qh += 32;
        }
    }
}

// src/ggml-quants.c:1275-1354 make_qkx2_quants(n = 16, nmax = 3, weights |x|, rmin -0.5, rdelta 0.1,
// nstep 15, use_mad = true), the (scale, min) search of one Q2_K sub-block by weighted absolute
// error. search_scale_min above is its n = 32 squared-error form and leaves the roundings to this
// file's compiler; here they are written out as the reference's x86 build (inlined into
// quantize_row_q2_K_reference, gcc -O3 -mfma) performs them. All of it is scalar code there and
// every product that feeds an add is contracted: sum_x = fma(w, x, sum_x) after a first rounded
// w0 x0; nearest_int(iscale (x - min)) = fma(iscale, x - min, 1.5 * 2^23); diff = fma(scale, l, min)
// - x; the error sums fma(w, |diff|, .); sum_l2 = fma(w l, l, .) and sum_xl = fma(w l, x, .) with
// w l rounded once; D = fma(sum_w, sum_l2, -(sum_l sum_l)), the min's numerator
// fma(sum_l2, sum_x, -(sum_l sum_xl)), the scale's fma(-sum_l, sum_x, sum_w sum_xl); and
// rmin + rdelta is + nmax is fma(0.1, is, -0.5) + 3.
float search_scale_min_mad16(const float * x, uint8_t * L, float * out_min) {
    constexpr int n = 16, nmax = 3, nstep = 15;
    uint8_t Laux[n];
    float w[n];
    for (int i = 0; i < n; ++i) w[i] = fabsf(x[i]);
    float lo = x[0], hi = x[0];
    float sum_w = w[0];
    float sum_x = mul_rn(w[0], x[0]);
    for (int i = 1; i < n; ++i) {
        if (x[i] < lo) lo = x[i];
        if (x[i] > hi) hi = x[i];
        sum_w += w[i];
        sum_x = fmaf(w[i], x[i], sum_x);
    }
    if (lo > 0) lo = 0;
    if (hi == lo) {
        memset(L, 0, n);
        *out_min = -lo;
        return 0.f;
    }
    float iscale = nmax / (hi - lo);
    float scale = 1 / iscale;
    float best = 0;
    for (int i = 0; i < n; ++i) {
        int l = rne_int_fma(iscale, x[i] - lo);
        L[i] = (uint8_t) clampv(l, 0, nmax);
        float diff = fabsf(fmaf(scale, (float) L[i], lo) - x[i]);
        best = fmaf(w[i], diff, best);
    }
    for (int is = 0; is <= nstep; ++is) {
        iscale = (fmaf(0.1f, (float) is, -0.5f) + (float) nmax) / (hi - lo);
        float sum_l = 0, sum_l2 = 0, sum_xl = 0;
        for (int i = 0; i < n; ++i) {
            int l = clampv(rne_int_fma(iscale, x[i] - lo), 0, nmax);
            Laux[i] = (uint8_t) l;
            const float wl = mul_rn(w[i], (float) l);
            sum_l2 = fmaf(wl, (float) l, sum_l2);
            sum_xl = fmaf(wl, x[i], sum_xl);
            sum_l += wl;
        }
        const float D = fmaf(sum_w, sum_l2, -mul_rn(sum_l, sum_l));
        if (D > 0) {
            float this_min = fmaf(sum_l2, sum_x, -mul_rn(sum_l, sum_xl)) / D;
            float this_scale;
            if (this_min > 0) {
                this_min = 0;
                this_scale = sum_xl / sum_l2;
            } else {
                this_scale = fmaf(-sum_l, sum_x, mul_rn(sum_w, sum_xl)) / D;
            }
            float mad = 0;
            for (int i = 0; i < n; ++i) {
                const float diff = fabsf(fmaf(this_scale, (float) Laux[i], this_min) - x[i]);
                mad = fmaf(w[i], diff, mad);
            }
            if (mad < best) {
                memcpy(L, Laux, n);
                best = mad;
                scale = this_scale;
                lo = this_min;
            }
        }
    }
    *out_min = -lo;
    return scale;
}

// the quants of Q2_K and Q3_K (and Q6_K's ql halves): byte qs[32 h + b] holds, at bit 2 t, the low
// two bits of element 128 h + 32 t + b
template <typename T> void pack_2bit(const T * L, uint8_t * qs) {
    for (int j = 0; j < kQKK; j += 128)
        for (int l = 0; l < 32; ++l)
            qs[j / 4 + l] = (uint8_t) (L[j + l] | (L[j + l + 32] << 2) | (L[j + l + 64] << 4) | (L[j + l + 96] << 6));
}

// src/ggml-quants.c:1369-1444 quantize_row_q2_K_reference. nearest_int(iscale * v) of the 4-bit
// scales and mins is the contracted fma; the final levels are nearest_int((x + dmin m) / d), where
// x + dmin m is one fma (dmin m is exact anyway: fp16 times a 4-bit integer) and the bias is added
// to the rounded quotient.
void quantize_q2_K_rows(const float * x, blk_q2_K * y, int64_t n) {
    uint8_t L[kQKK];
    float mins[kQKK / 16], scales[kQKK / 16];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        float max_scale = 0, max_min = 0;
        for (int j = 0; j < kQKK / 16; ++j) {
            scales[j] = search_scale_min_mad16(x + 16 * j, L + 16 * j, &mins[j]);
            if (scales[j] > max_scale) max_scale = scales[j];
            if (mins[j] > max_min) max_min = mins[j];
        }
        if (max_scale > 0) {
            const float iscale = 15.f / max_scale;
            for (int j = 0; j < kQKK / 16; ++j) y[b].scales[j] = (uint8_t) rne_int_fma(iscale, scales[j]);
            y[b].d = ggml_fp32_to_fp16(max_scale / 15.f);
        } else {
            memset(y[b].scales, 0, kQKK / 16);
            y[b].d = ggml_fp32_to_fp16(0.f);
        }
        if (max_min > 0) {
            const float iscale = 15.f / max_min;
            for (int j = 0; j < kQKK / 16; ++j) y[b].scales[j] |= (uint8_t) (rne_int_fma(iscale, mins[j]) << 4);
            y[b].dmin = ggml_fp32_to_fp16(max_min / 15.f);
        } else {
            y[b].dmin = ggml_fp32_to_fp16(0.f);
        }
        for (int j = 0; j < kQKK / 16; ++j) {
            const float d = ggml_fp16_to_fp32(y[b].d) * (float) (y[b].scales[j] & 0xF);
            if (!d) continue;
            const float dmin = ggml_fp16_to_fp32(y[b].dmin), m = (float) (y[b].scales[j] >> 4);
            for (int ii = 0; ii < 16; ++ii) {
                int l = rne_int(fmaf(dmin, m, x[16 * j + ii]) / d);
                L[16 * j + ii] = (uint8_t) clampv(l, 0, 3);
            }
        }
        pack_2bit(L, y[b].qs);
    }
}

// src/ggml-quants.c:1173-1230 make_q3_quants(n = 16, nmax = 4, do_rmse = true): the symmetric scale
// of one Q3_K sub-block, weights x^2, refined by up to five passes that move one level at a time.
// Roundings as the reference's x86 build performs them (inlined into quantize_row_q3_K_reference,
// scalar throughout): w x and w l are rounded products, then sumlx = fma(w x, l, sumlx) and
// suml2 = fma(w l, l, suml2); in the refinement slx = fma(-(w x), l, sumlx), sl2 = fma(-(w l), l,
// suml2), the candidate level nearest_int((x sl2) / slx) with the bias added to the rounded
// quotient, and the updates again fma(w x, new_l, slx) / fma(w new_l, new_l, sl2); the comparison
// multiplies (slx slx) suml2 and (sumlx sumlx) sl2 from the left. L gets the levels + 4.
float search_scale_q3(const float * x, int8_t * L) {
    constexpr int n = 16, nmax = 4;
    float max = 0;
    float amax = 0;
    for (int i = 0; i < n; ++i) {
        float ax = fabsf(x[i]);
        if (ax > amax) { amax = ax; max = x[i]; }
    }
    if (!amax) {  // all zero
        for (int i = 0; i < n; ++i) L[i] = 0;
        return 0.f;
    }
    const float iscale = -nmax / max;
    float sumlx = 0;
    float suml2 = 0;
    for (int i = 0; i < n; ++i) {
        int l = clampv(rne_int_fma(iscale, x[i]), -nmax, nmax - 1);
        L[i] = (int8_t) l;
        const float w = mul_rn(x[i], x[i]);
        sumlx = fmaf(mul_rn(w, x[i]), (float) l, sumlx);
        suml2 = fmaf(mul_rn(w, (float) l), (float) l, suml2);
    }
    for (int itry = 0; itry < 5; ++itry) {
        int n_changed = 0;
        for (int i = 0; i < n; ++i) {
            const float w = mul_rn(x[i], x[i]);
            const float wx = mul_rn(w, x[i]);
            const float lf = (float) L[i];
            float slx = fmaf(-wx, lf, sumlx);
            if (slx > 0) {
                float sl2 = fmaf(-mul_rn(w, lf), lf, suml2);
                int new_l = clampv(rne_int(mul_rn(x[i], sl2) / slx), -nmax, nmax - 1);
                if (new_l != L[i]) {
                    const float nf = (float) new_l;
                    sl2 = fmaf(mul_rn(w, nf), nf, sl2);
                    slx = fmaf(wx, nf, slx);
                    if (sl2 > 0 && mul_rn(mul_rn(slx, slx), suml2) > mul_rn(mul_rn(sumlx, sumlx), sl2)) {
                        L[i] = (int8_t) new_l;
                        sumlx = slx;
                        suml2 = sl2;
                        ++n_changed;
                    }
                }
            }
        }
        if (!n_changed) break;
    }
    for (int i = 0; i < n; ++i) L[i] = (int8_t) (L[i] + nmax);
    return sumlx / suml2;
}

// the 6-bit scale of Q3_K sub-block j (0..63, the value + 32): low four bits in the nibbles of
// scales[0..7], upper two bits in scales[8 + j % 4] at bit 2 (j / 4)
inline int q3_scale(const uint8_t * scales, int j) {
    const int lo = j < 8 ? scales[j] & 0xF : scales[j - 8] >> 4;
    return lo | (((scales[8 + j % 4] >> (2 * (j / 4))) & 3) << 4);
}

// src/ggml-quants.c:1766-1877 quantize_row_q3_K_reference. nearest_int(iscale * scale) is the
// contracted fma, cut to int8_t before the clamp as there; the final levels are
// nearest_int(x / d) with the bias added to the rounded quotient. A sub-block whose d * sc is zero
// keeps the levels of the search.
void quantize_q3_K_rows(const float * x, blk_q3_K * y, int64_t n) {
    int8_t L[kQKK];
    float scales[kQKK / 16];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        float max_scale = 0;
        float amax = 0;
        for (int j = 0; j < kQKK / 16; ++j) {
            scales[j] = search_scale_q3(x + 16 * j, L + 16 * j);
            const float scale = fabsf(scales[j]);
            if (scale > amax) {
                amax = scale;
                max_scale = scales[j];
            }
        }
        memset(y[b].scales, 0, 12);
        if (max_scale) {
            const float iscale = -32.f / max_scale;
            for (int j = 0; j < kQKK / 16; ++j) {
                int8_t l = (int8_t) rne_int_fma(iscale, scales[j]);
                l = (int8_t) (clampv((int) l, -32, 31) + 32);
                if (j < 8) y[b].scales[j] = (uint8_t) (l & 0xF);
                else y[b].scales[j - 8] |= (uint8_t) ((l & 0xF) << 4);
                l = (int8_t) (l >> 4);
                y[b].scales[j % 4 + 8] |= (uint8_t) (l << (2 * (j / 4)));
            }
            y[b].d = ggml_fp32_to_fp16(1 / iscale);
        } else {
            y[b].d = ggml_fp32_to_fp16(0.f);
        }
        for (int j = 0; j < kQKK / 16; ++j) {
            const float d = ggml_fp16_to_fp32(y[b].d) * (float) (q3_scale(y[b].scales, j) - 32);
            if (!d) continue;
            for (int ii = 0; ii < 16; ++ii) {
                int l = rne_int(x[16 * j + ii] / d);
                L[16 * j + ii] = (int8_t) (clampv(l, -4, 3) + 4);
            }
        }
        // bit 4 h + t of hmask[b]: the high bit of element 128 h + 32 t + b
        memset(y[b].hmask, 0, kQKK / 8);
        for (int j = 0; j < kQKK; ++j) {
            if (L[j] > 3) {
                y[b].hmask[j % 32] |= (uint8_t) (1u << (j / 32));
                L[j] = (int8_t) (L[j] - 4);
            }
        }
        pack_2bit(L, y[b].qs);
    }
}

// ---- IQ4_NL / IQ4_XS: 4-bit indices into a fixed non-linear codebook (src/ggml-quants.c:3321)
constexpr int8_t kValuesIQ4NL[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};

// src/ggml-quants.c:14166-14175 best_index_int8(16, kvalues_iq4nl, x): the index of the level nearest
// to x, the upper one on a tie
inline int iq4_best_index(float x) {
    const int8_t * val = kValuesIQ4NL;
    if (x <= val[0]) return 0;
    if (x >= val[15]) return 15;
    int ml = 0, mu = 15;
    while (mu - ml > 1) {
        const int mav = (ml + mu) / 2;
        if (x < val[mav]) mu = mav; else ml = mav;
    }
    return x - val[mu - 1] < val[mu] - x ? mu - 1 : mu;
}

// src/ggml-quants.c:14192-14246, the scale search of one 32-element block in
// quantize_row_iq4_nl_impl(quant_weights = NULL, ntry = 7): weights x^2, a first scale -max / -127,
// then the fifteen candidates id = (itry - 127) / max, itry = -7..7, the best by sumqx^2 / sumq2.
// Roundings as the reference's x86 build performs them (gcc -O3 -mfma; the same in
// quantize_row_iq4_nl_impl.constprop, IQ4_NL, and inlined into quantize_iq4_xs): w = x x and w q are
// rounded products, then sumqx = fma(w q, x, sumqx) and sumq2 = fma(w q, q, sumq2); id x, sumqx sumqx,
// best sumq2 and d sumqx are plain products. Returns 0 for an all-zero block.
float iq4_block_scale(const float * xb) {
    float w[32];
    float amax = 0, max = 0;
    for (int j = 0; j < 32; ++j) {
        w[j] = mul_rn(xb[j], xb[j]);
        const float ax = fabsf(xb[j]);
        if (ax > amax) { amax = ax; max = xb[j]; }
    }
    if (!amax) return 0.f;
    auto sums = [&](float id, float & sumqx, float & sumq2) {
        sumqx = sumq2 = 0;
        for (int j = 0; j < 32; ++j) {
            const float q = (float) kValuesIQ4NL[iq4_best_index(mul_rn(id, xb[j]))];
            const float wq = mul_rn(w[j], q);
            sumqx = fmaf(wq, xb[j], sumqx);
            sumq2 = fmaf(wq, q, sumq2);
        }
    };
    float sumqx, sumq2;
    float d = -max / (float) kValuesIQ4NL[0];
    sums(1 / d, sumqx, sumq2);
    d = sumqx / sumq2;
    float best = mul_rn(d, sumqx);
    for (int itry = -7; itry <= 7; ++itry) {
        sums((float) (itry + kValuesIQ4NL[0]) / max, sumqx, sumq2);
        if (sumq2 > 0 && mul_rn(sumqx, sumqx) > mul_rn(best, sumq2)) {
            d = sumqx / sumq2;
            best = mul_rn(d, sumqx);
        }
    }
    return d;
}

// byte j of a 32-element block: index of element j | index of element 16 + j << 4
inline void iq4_pack(const uint8_t * L, uint8_t * qs) {
    for (int j = 0; j < 16; ++j) qs[j] = (uint8_t) (L[j] | (L[16 + j] << 4));
}

// src/ggml-quants.c:14288-14308 quantize_iq4_nl: d = fp16 of the searched scale (not re-read), the
// indices from id = 1 / scale (0 for a zero scale: every index 8, the level 1)
void quantize_iq4_nl_rows(const float * x, blk_iq4_nl * y, int64_t n) {
    uint8_t L[32];
    for (int64_t b = 0; b < n / 32; ++b, x += 32) {
        const float scale = iq4_block_scale(x);
        y[b].d = ggml_fp32_to_fp16(scale);
        const float id = scale ? 1 / scale : 0.f;
        for (int j = 0; j < 32; ++j) L[j] = (uint8_t) iq4_best_index(mul_rn(id, x[j]));
        iq4_pack(L, y[b].qs);
    }
}

// src/ggml-quants.c:14330-14352 quantize_iq4_xs, the second pass of quantize_row_iq4_nl_impl
// (:14248-14270): d = -max_scale / 32 of the block scale of largest magnitude, the 6-bit
// l = clamp(nearest_int(id scale), -32, 31) with nearest_int's product contracted into the bias add,
// the indices from idl = 1 / (d l) with d the f32 value (0 for a zero d l), l + 32 packed: low four
// bits in the nibbles of scales_l, upper two at bit 2 ib of scales_h. An all-zero superblock has
// d = -0.0, l = 0: every l + 32 = 32, scales_h 0xAAAA.
void quantize_iq4_xs_rows(const float * x, blk_iq4_xs * y, int64_t n) {
    uint8_t L[32];
    float scales[kQKK / 32];
    for (int64_t b = 0; b < n / kQKK; ++b, x += kQKK) {
        float max_scale = 0, amax_scale = 0;
        for (int ib = 0; ib < kQKK / 32; ++ib) {
            scales[ib] = iq4_block_scale(x + 32 * ib);
            const float abs_d = fabsf(scales[ib]);
            if (abs_d > amax_scale) { amax_scale = abs_d; max_scale = scales[ib]; }
        }
        const float d = -max_scale / 32;
        y[b].d = ggml_fp32_to_fp16(d);
        y[b].scales_h = 0;
        const float id = d ? 1 / d : 0.f;
        for (int ib = 0; ib < kQKK / 32; ++ib) {
            int l = clampv(rne_int_fma(id, scales[ib]), -32, 31);
            const float dl = mul_rn(d, (float) l);
            const float idl = dl ? 1 / dl : 0.f;
            for (int j = 0; j < 32; ++j) L[j] = (uint8_t) iq4_best_index(mul_rn(idl, x[32 * ib + j]));
            iq4_pack(L, y[b].qs + 16 * ib);
            l += 32;
            if (ib % 2 == 0) y[b].scales_l[ib / 2] = (uint8_t) (l & 0xF);
            else y[b].scales_l[ib / 2] |= (uint8_t) ((l & 0xF) << 4);
            y[b].scales_h |= (uint16_t) ((l >> 4) << (2 * ib));
        }
    }
}

} // namespace

extern "C" {

void ggml_quantize_init(enum ggml_type) {}
void ggml_quantize_free(void) {}

bool ggml_quantize_requires_imatrix(enum ggml_type type) {
    return type == GGML_TYPE_IQ2_XXS || type == GGML_TYPE_IQ2_XS || type == GGML_TYPE_IQ1_S;
}

size_t ggml_quantize_chunk(enum ggml_type type, const float * src, void * dst, int64_t start, int64_t nrows,
                           int64_t n_per_row, const float * imatrix) {
    GGML_ASSERT(start % ggml_blck_size(type) == 0);
    GGML_ASSERT(start % n_per_row == 0);
    const int64_t n = nrows * n_per_row;
    const size_t row_size = ggml_row_size(type, n_per_row);
    char * out = (char *) dst + (start / n_per_row) * row_size;
    const float * in = src + start;
    if (imatrix != NULL && type != GGML_TYPE_Q8_0 && type != GGML_TYPE_F16 && type != GGML_TYPE_BF16 && type != GGML_TYPE_F32) {
        GGML_ASSERT(!"importance-matrix quantization is not supported by this runtime");
    }
    switch (type) {
        case GGML_TYPE_Q4_0: quantize_q4_0_rows(in, (blk_q4_0 *) out, n); break;
        case GGML_TYPE_Q4_1: quantize_q4_1_rows(in, (blk_q4_1 *) out, n); break;
        case GGML_TYPE_Q5_0: quantize_q5_0_rows(in, (blk_q5_0 *) out, n); break;
        case GGML_TYPE_Q5_1: quantize_q5_1_rows(in, (blk_q5_1 *) out, n); break;
        case GGML_TYPE_Q8_0: quantize_q8_0_rows(in, (blk_q8_0 *) out, n); break;
        case GGML_TYPE_Q2_K: quantize_q2_K_rows(in, (blk_q2_K *) out, n); break;
        case GGML_TYPE_Q3_K: quantize_q3_K_rows(in, (blk_q3_K *) out, n); break;
        case GGML_TYPE_Q4_K: quantize_q4_K_rows(in, (blk_q4_K *) out, n); break;
        case GGML_TYPE_Q5_K: quantize_q5_K_rows(in, (blk_q5_K *) out, n); break;
        case GGML_TYPE_Q6_K: quantize_q6_K_rows(in, (blk_q6_K *) out, n); break;
        case GGML_TYPE_IQ4_NL: quantize_iq4_nl_rows(in, (blk_iq4_nl *) out, n); break;
        case GGML_TYPE_IQ4_XS: quantize_iq4_xs_rows(in, (blk_iq4_xs *) out, n); break;
        case GGML_TYPE_F16: ggml_fp32_to_fp16_row(in, (ggml_fp16_t *) out, n); break;
        case GGML_TYPE_BF16: ggml_fp32_to_bf16_row(in, (ggml_bf16_t *) out, n); break;
        case GGML_TYPE_F32: memcpy(out, in, (size_t) n * sizeof(float)); break;
        default: GGML_ASSERT(!"ggml_quantize_chunk: type not supported by this runtime");
    }
    return (size_t) nrows * row_size;
}

} // extern "C"
