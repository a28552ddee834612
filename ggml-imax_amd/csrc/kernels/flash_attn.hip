// flash_attn.hip -- GGML_OP_FLASH_ATTN_EXT on gfx950 (src/ggml.c:15572-15751): fused attention with an
// f16 K/V cache read through strided views, grouped-query heads, an f16 mask and ALiBi slopes.
//
//   s[ic] = dot(k[ic], f16(q)) * scale + slope * mask[iq1][ic]        (all f32; -inf mask: key skipped)
//   dst[:, iq2, iq1, iq3] = sum_ic softmax(s)[ic] * v[ic]              (f32 accumulation, one division)
//
// Two kernels. Fewer than kFaMmaMinN queries (decode, batched decode, short chunks): k_fa_vec, below.
// Prompts: k_fa_mma, f16 MFMA over KV tiles staged in LDS (described at the kernel).
//
// k_fa_vec: K/V go straight to VGPRs as 16-byte loads, nothing is staged in LDS.
// Heads that share a K head and a V head form a group (G = gcd(nh / nh_k, nh / nh_v) heads); the rows
// of a group are its (query, head in group) pairs. A workgroup takes R <= 8 rows of one group and a
// range of keys, so K/V of that range are read once for all R rows. Inside the workgroup a key belongs
// to LPK = 8 / 16 / 32 lanes (8 head dimensions per lane), a wave holds 64 / LPK keys per pass, and
// every (wave, key slot) keeps its own online-softmax stream (m, l, O) in registers. The streams are
// merged at the end: across the slots of a wave by cross-lane exchange, across the four waves through
// LDS in wave order. With more than one key range (mi_fa_splits) the workgroup stores (m, l, O)
// to the partials and k_fa_combine merges the ranges in index order -- no atomics, so the result does
// not depend on scheduling.
//
// Bounds: a lane loads K/V only for keys ic < kv and for head dimensions < D (the lanes past D in a
// key's LPK idle and count as zeros), the mask only at [iq1 < N][ic < kv], and writes dst rows < N only.

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

namespace {

constexpr int kFaWaves = 4;
constexpr int kFaMaxRows = 8;      // rows of one workgroup at most (16 leave one wave per SIMD: 256 VGPRs + 113 AGPRs)
constexpr int kFaMinSplitKeys = 128;
constexpr int kFaTargetWgs = 1024; // four workgroups per CU
constexpr int kFaMmaMinN = 32;     // queries from which the MFMA kernel runs: a wave's 32 rows are all real

typedef _Float16 fa_half2 __attribute__((ext_vector_type(2)));
typedef _Float16 fa_half8 __attribute__((ext_vector_type(8)));
typedef float fa_float16 __attribute__((ext_vector_type(16)));

struct fa_args {
    mi_fa_desc d;
    int G, ngrp, rk2, rv2, rk3, rv3;  // group size, groups per ne3 index, broadcast factors
    int nblk;                         // row blocks per group
    int splits, split_keys;
    int n_head_log2;
    float m0, m1;
    bool mma;                         // k_fa_mma runs (then splits == 1)
};

__host__ __device__ inline int fa_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

template <bool AL>
__device__ __forceinline__ uint4 fa_load16(const char * p) {
    if (AL) return *(const uint4 *) p;
    const uint16_t * h = (const uint16_t *) p;
    uint4 r;
    r.x = h[0] | ((uint32_t) h[1] << 16);
    r.y = h[2] | ((uint32_t) h[3] << 16);
    r.z = h[4] | ((uint32_t) h[5] << 16);
    r.w = h[6] | ((uint32_t) h[7] << 16);
    return r;
}

__device__ __forceinline__ fa_half2 fa_as_h2(uint32_t u) {
    return __builtin_bit_cast(fa_half2, u);
}

__device__ __forceinline__ float fa_exp(float x) { return __expf(x); }

// merges the stream (mo, lo, oo) into (m, l, o); a stream without keys has m = -inf, l = 0, o = 0
__device__ __forceinline__ void fa_merge_scales(float m, float mo, float & mn, float & a, float & b) {
    mn = fmaxf(m, mo);
    const bool none = mn == -INFINITY;
    a = none ? 1.0f : fa_exp(m - mn);
    b = none ? 0.0f : fa_exp(mo - mn);
}

__device__ __forceinline__ void fa_row_of(const fa_args & a, int grp, int r, int & iq1, int & h) {
    iq1 = r / a.G;
    h = grp * a.G + r % a.G;
}

// the sum over the LPK lanes of a key, in every one of them: DPP inside a row of 16 lanes (the whole wave
// must be active), one cross-lane exchange more for 32 lanes
template <int LPK>
__device__ __forceinline__ float fa_group_sum(float v) {
    auto f = [](int x) { return __int_as_float(x); };
    auto i = [](float x) { return __float_as_int(x); };
    v += f(mi_dpp<MI_DPP_QP_1032>(0, i(v)));
    v += f(mi_dpp<MI_DPP_QP_2301>(0, i(v)));
    v += f(mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, i(v)));
    if (LPK >= 16) v += f(mi_dpp<MI_DPP_ROW_MIRROR>(0, i(v)));
    if (LPK >= 32) v += __shfl_xor(v, 16);
    return v;
}

template <int R, int LPK, bool AL>
__global__ __launch_bounds__(64 * kFaWaves) void k_fa_vec(const fa_args a) {
    constexpr int KPW = 64 / LPK;   // keys of a wave per pass
    constexpr int DP = LPK * 8;     // head size padded to the lanes of a key
    __shared__ float sm[(kFaWaves - 1) * R * (DP + 2)];

    const mi_fa_desc & d = a.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane % LPK, g = lane / LPK;
    const int split = blockIdx.x, blk = blockIdx.y;
    const int grp = blockIdx.z % a.ngrp, i3 = blockIdx.z / a.ngrp;
    const int rtot = d.N * a.G;
    const bool act = c * 8 < d.D;

    fa_half2 qh[R][4];
    float slope[R];
    int qrow[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        int iq1, h;
        fa_row_of(a, grp, min(blk * R + r, rtot - 1), iq1, h);
        float qf[8] = {};
        if (act) {
            const float * pq = (const float *) (d.q + (size_t) iq1 * d.nbq1 + (size_t) h * d.nbq2 + (size_t) i3 * d.nbq3) + c * 8;
#pragma unroll
            for (int j = 0; j < 8; j++) qf[j] = pq[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            fa_half2 t;
            t.x = (_Float16) qf[2 * j];  // round to nearest even, as GGML_FP32_TO_FP16
            t.y = (_Float16) qf[2 * j + 1];
            qh[r][j] = t;
        }
        slope[r] = 1.0f;
        if (d.max_bias > 0.0f) {
            slope[r] = h < a.n_head_log2 ? powf(a.m0, (float) (h + 1)) : powf(a.m1, (float) (2 * (h - a.n_head_log2) + 1));
        }
        qrow[r] = iq1;
    }

    const int h0 = grp * a.G;
    const char * kb = d.k + (size_t) (h0 / a.rk2) * d.nbk2 + (size_t) (i3 / a.rk3) * d.nbk3 + c * 16;
    const char * vb = d.v + (size_t) (h0 / a.rv2) * d.nbv2 + (size_t) (i3 / a.rv3) * d.nbv3 + c * 16;

    float m[R], l[R], o[R][8];
#pragma unroll
    for (int r = 0; r < R; r++) {
        m[r] = -INFINITY;
        l[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) o[r][j] = 0.0f;
    }

    const int kbeg = split * a.split_keys;
    const int kend = min(d.kv, kbeg + a.split_keys);
    // U keys of a stream at a time: all their loads are issued before the first use, and O is rescaled once
    constexpr int U = R <= 4 ? 4 : 2;
    for (int ic0 = kbeg + wave * KPW; ic0 < kend; ic0 += kFaWaves * KPW * U) {  // wave-uniform bounds
        uint4 kk[U], vv[U];
        int ic[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            ic[u] = ic0 + u * kFaWaves * KPW + g;
            ok[u] = ic[u] < kend;
            kk[u] = vv[u] = {0, 0, 0, 0};
            if (ok[u] && act) {
                kk[u] = fa_load16<AL>(kb + (size_t) ic[u] * d.nbk1);
                vv[u] = fa_load16<AL>(vb + (size_t) ic[u] * d.nbv1);
            }
        }
        float s[U][R];  // first the mask term, then the score
        bool anyskip = false;
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                float mv = ok[u] ? 0.0f : -INFINITY;
                if (d.mask && ok[u]) mv = slope[r] * mi_h2f(*(const uint16_t *) (d.mask + (size_t) qrow[r] * d.nbm1 + (size_t) ic[u] * 2));
                s[u][r] = mv;
                anyskip |= ok[u] && mv == -INFINITY;
            }
        }
        // 0 * v is not 0 for an inf / NaN v: only a masked key whose V chunk holds one needs the select below
        bool bad = false;
        if (__any(anyskip)) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t w[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                for (int i = 0; i < 4; i++) bad |= (w[i] & 0x7c00u) == 0x7c00u || (w[i] & 0x7c000000u) == 0x7c000000u;
            }
        }
        const bool slow = __any(bad);
        float vf[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) {
            float t[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                float x = __builtin_amdgcn_fdot2(fa_as_h2(kk[u].x), qh[r][0], 0.0f, false);
                x = __builtin_amdgcn_fdot2(fa_as_h2(kk[u].y), qh[r][1], x, false);
                x = __builtin_amdgcn_fdot2(fa_as_h2(kk[u].z), qh[r][2], x, false);
                t[r] = __builtin_amdgcn_fdot2(fa_as_h2(kk[u].w), qh[r][3], x, false);
            }
#pragma unroll
            for (int r = 0; r < R; r++) t[r] = fa_group_sum<LPK>(t[r]);
            // a key past the range or masked with -inf contributes nothing, whatever K and V hold there
#pragma unroll
            for (int r = 0; r < R; r++) s[u][r] = s[u][r] == -INFINITY ? -INFINITY : t[r] * d.scale + s[u][r];
            const fa_half2 v0 = fa_as_h2(vv[u].x), v1 = fa_as_h2(vv[u].y), v2 = fa_as_h2(vv[u].z), v3 = fa_as_h2(vv[u].w);
            vf[u][0] = (float) v0.x; vf[u][1] = (float) v0.y; vf[u][2] = (float) v1.x; vf[u][3] = (float) v1.y;
            vf[u][4] = (float) v2.x; vf[u][5] = (float) v2.y; vf[u][6] = (float) v3.x; vf[u][7] = (float) v3.y;
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            float mn = m[r];
#pragma unroll
            for (int u = 0; u < U; u++) mn = fmaxf(mn, s[u][r]);
            const bool none = mn == -INFINITY;
            const float sc = none ? 1.0f : fa_exp(m[r] - mn);
            float p[U], sum = 0.0f;
#pragma unroll
            for (int u = 0; u < U; u++) {
                p[u] = none ? 0.0f : fa_exp(s[u][r] - mn);  // a skipped key: exp(-inf) = 0
                sum += p[u];
            }
            l[r] = l[r] * sc + sum;
            m[r] = mn;
            if (slow) {  // wave-uniform
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    float acc = o[r][j] * sc;
#pragma unroll
                    for (int u = 0; u < U; u++) acc += s[u][r] == -INFINITY ? 0.0f : p[u] * vf[u][j];
                    o[r][j] = acc;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    float acc = o[r][j] * sc;
#pragma unroll
                    for (int u = 0; u < U; u++) acc = fmaf(p[u], vf[u][j], acc);
                    o[r][j] = acc;
                }
            }
        }
    }

    // the key slots of a wave (rolled over the distance, a row at a time: the exchange needs few registers)
#pragma unroll 1
    for (int off = LPK; off < 64; off <<= 1) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            __builtin_amdgcn_sched_barrier(0);
            const float mo = __shfl_xor(m[r], off), lo = __shfl_xor(l[r], off);
            float mn, sa, sb;
            fa_merge_scales(m[r], mo, mn, sa, sb);
            l[r] = l[r] * sa + lo * sb;
            m[r] = mn;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float oo = __shfl_xor(o[r][j], off);
                o[r][j] = o[r][j] * sa + oo * sb;
            }
        }
    }
    (void) KPW;

    // the waves, in wave order
    if (wave > 0 && g == 0) {
        float * w = sm + (size_t) (wave - 1) * R * (DP + 2);
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int j = 0; j < 8; j++) w[r * (DP + 2) + c * 8 + j] = o[r][j];
            if (c == 0) {
                w[r * (DP + 2) + DP] = m[r];
                w[r * (DP + 2) + DP + 1] = l[r];
            }
        }
    }
    __syncthreads();
    if (wave > 0 || g > 0) return;
#pragma unroll 1
    for (int w = 0; w < kFaWaves - 1; w++) {
        const float * p = sm + (size_t) w * R * (DP + 2);
#pragma unroll
        for (int r = 0; r < R; r++) {
            __builtin_amdgcn_sched_barrier(0);
            float mn, sa, sb;
            fa_merge_scales(m[r], p[r * (DP + 2) + DP], mn, sa, sb);
            l[r] = l[r] * sa + p[r * (DP + 2) + DP + 1] * sb;
            m[r] = mn;
#pragma unroll
            for (int j = 0; j < 8; j++) o[r][j] = o[r][j] * sa + p[r * (DP + 2) + c * 8 + j] * sb;
        }
    }

#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = blk * R + r;
        if (row >= rtot) break;
        if (a.splits == 1) {
            if (!act) continue;
            int iq1, h;
            fa_row_of(a, grp, row, iq1, h);
            float * y = d.dst + (((size_t) i3 * d.N + iq1) * d.nh + h) * d.D + c * 8;
#pragma unroll
            for (int j = 0; j < 8; j++) y[j] = o[r][j] / l[r];  // no unmasked key: 0 / 0 = NaN, as the reference
        } else {
            float * y = d.part + ((((size_t) blockIdx.z * a.nblk + blk) * a.splits + split) * R + r) * (DP + 2);
#pragma unroll
            for (int j = 0; j < 8; j++) y[c * 8 + j] = o[r][j];
            if (c == 0) {
                y[DP] = m[r];
                y[DP + 1] = l[r];
            }
        }
    }
}

// ---- prompts: f16 MFMA ---------------------------------------------------------------------------------
// A workgroup of 2 or 4 waves takes 32 query rows of one head per wave and walks the keys in tiles of
// KT = 64 (32 at head size 256, whose O accumulators take 128 registers). Both products run
// transposed on v_mfma_f32_32x32x16_f16, so a lane owns one query row throughout:
//   S^T [key x q] = K [key x d] . Q^T [d x q]     A = K from LDS, B = Q (f16, in registers for the whole kernel)
//   O^T [d x q]  += V^T [d x key] . P^T [key x q]  A = V^T from LDS, B = P rounded to f16
// Lane (q = lane % 32, hi = lane / 32) holds S^T / O^T rows (r % 4) + 8 (r / 4) + 4 hi, r < 16, of column
// q: the row maximum and sum are in-lane reductions plus one exchange with lane ^ 32, and m, l and the
// rescale factor are scalars of the lane. The 16 probabilities a lane holds of a 32-key block are, in
// order, the B operand of two MFMAs whose contraction index runs over those very keys, so P never leaves
// its registers; V is stored transposed in LDS with each 32-key block's columns in that order
// (fa_vslot), 8 consecutive halves per MFMA operand. K rows and V^T rows are padded by 16 bytes, which
// spreads the 16-byte reads of 32 consecutive rows over the banks. Head sizes 80 and 112 are padded
// to 96 / 128 with zeros in LDS and in Q's registers; keys past kv are zeros in LDS and -inf in S.
// Before a tile is staged every wave reads its mask block (the values it needs for S anyway); a tile
// all of whose mask values are -inf for all rows of the workgroup is not staged (a workgroup-uniform
// decision, __syncthreads_or), and a wave whose own rows are all masked skips the tile's MFMAs, so a
// causal prompt does about half the work. O and l accumulate in f32; one division at the end.
// A masked key contributes p = 0 exactly, which the PV MFMA multiplies with the key's V row: K / V rows
// of masked keys inside [0, kv) must hold finite values here (k_fa_vec does not read them at all).
__device__ __forceinline__ int fa_vslot(int kk) {
    const int k32 = kk & 31, j = k32 >> 4, rem = k32 & 15;
    const int i = ((rem >> 3) << 2) | (rem & 3), hi = (rem >> 2) & 1;
    return (kk & ~31) + j * 16 + hi * 8 + i;
}

template <int DP, int KT, bool AL>
__global__ __launch_bounds__(256) void k_fa_mma(const fa_args a) {
    constexpr int KB = KT / 32, DC = DP / 16, DB = DP / 32;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[KT][DP + 8];
    __shared__ __attribute__((aligned(16))) _Float16 Vt[DP][KT + 8];

    const mi_fa_desc & d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int ql = lane & 31, hi = lane >> 5;
    const int h = blockIdx.y, i3 = blockIdx.z;
    const int qrow = (blockIdx.x * nw + wave) * 32 + ql;
    const bool qok = qrow < d.N;

    fa_half8 qreg[DC];
    {
        const float * pq = (const float *) (d.q + (size_t) min(qrow, d.N - 1) * d.nbq1 + (size_t) h * d.nbq2 + (size_t) i3 * d.nbq3);
#pragma unroll
        for (int dc = 0; dc < DC; dc++) {
            const int d0 = dc * 16 + 8 * hi;
            const bool in = qok && d0 < d.D;  // D is a multiple of 8: a chunk lies wholly inside or outside
#pragma unroll
            for (int i = 0; i < 8; i++) qreg[dc][i] = (_Float16) (in ? pq[d0 + i] : 0.0f);  // round to nearest even
        }
    }
    float slope = 1.0f;
    if (d.max_bias > 0.0f) slope = h < a.n_head_log2 ? powf(a.m0, (float) (h + 1)) : powf(a.m1, (float) (2 * (h - a.n_head_log2) + 1));
    const uint16_t * mrow = d.mask && qok ? (const uint16_t *) (d.mask + (size_t) qrow * d.nbm1) : nullptr;
    const char * kb0 = d.k + (size_t) (h / a.rk2) * d.nbk2 + (size_t) (i3 / a.rk3) * d.nbk3;
    const char * vb0 = d.v + (size_t) (h / a.rv2) * d.nbv2 + (size_t) (i3 / a.rv3) * d.nbv3;

    fa_float16 O[DB];
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
        for (int r = 0; r < 16; r++) O[db][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;  // l: this lane's keys only; the two halves are added at the end

    for (int k0 = 0; k0 < d.kv; k0 += KT) {
        // the mask block of this wave's rows: slope * mask, 0 without a mask, -inf past N or kv
        float mv[KB][16];
        bool any = false;
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                float x = -INFINITY;
                if (qok && key < d.kv) x = mrow ? slope * mi_h2f(mrow[key]) : 0.0f;
                mv[kb][r] = x;
                any |= x != -INFINITY;
            }
        }
        const bool wave_any = __ballot(any) != 0;
        // (also the barrier behind the previous tile's LDS reads)
        if (!__syncthreads_or(wave_any)) continue;

        for (int t = tid; t < KT * (DP / 8); t += blockDim.x) {
            const int key = t / (DP / 8), c = t % (DP / 8);
            uint4 kk = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
            if (k0 + key < d.kv && c * 8 < d.D) {
                kk = fa_load16<AL>(kb0 + (size_t) (k0 + key) * d.nbk1 + c * 16);
                vv = fa_load16<AL>(vb0 + (size_t) (k0 + key) * d.nbv1 + c * 16);
            }
            *(uint4 *) &Ks[key][c * 8] = kk;
            const int slot = fa_vslot(key);
            const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const fa_half2 p2 = fa_as_h2(w[i]);
                Vt[c * 8 + 2 * i][slot] = p2.x;
                Vt[c * 8 + 2 * i + 1][slot] = p2.y;
            }
        }
        __syncthreads();
        if (!wave_any) continue;  // wave-uniform; the next barrier is the __syncthreads_or above

        float s[KB][16];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
            fa_float16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
            for (int dc = 0; dc < DC; dc++) {
                const fa_half8 ka = *(const fa_half8 *) &Ks[kb * 32 + ql][dc * 16 + 8 * hi];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka, qreg[dc], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[kb][r] = mv[kb][r] == -INFINITY ? -INFINITY : acc[r] * d.scale + mv[kb][r];
                mx = fmaxf(mx, s[kb][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const bool none = mn == -INFINITY;
        const float sc = none ? 1.0f : fa_exp(m - mn);
        fa_half8 P[KB][2];
        float sum = 0.0f;
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float p = none ? 0.0f : fa_exp(s[kb][r] - mn);
                sum += p;
                P[kb][r >> 3][r & 7] = (_Float16) p;
            }
        }
        l = l * sc + sum;
        m = mn;
#pragma unroll
        for (int db = 0; db < DB; db++) {
#pragma unroll
            for (int r = 0; r < 16; r++) O[db][r] *= sc;
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const fa_half8 va = *(const fa_half8 *) &Vt[db * 32 + ql][kb * 32 + j * 16 + hi * 8];
                    O[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, P[kb][j], O[db], 0, 0, 0);
                }
            }
        }
    }

    l += __shfl_xor(l, 32);
    if (!qok) return;
    float * y = d.dst + (((size_t) i3 * d.N + qrow) * d.nh + h) * d.D;
#pragma unroll
    for (int db = 0; db < DB; db++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int dd = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (dd < d.D) y[dd] = O[db][r] / l;  // no unmasked key: 0 / 0 = NaN, as the reference
        }
    }
}

// merges the key ranges of one row in index order; R, DP as the split kernel's. One workgroup per
// (group, row block, row): the weights exp(m_s - M) go to LDS, one per thread; then a thread per head
// dimension adds its column over the ranges, index order, the loads independent of one another.
constexpr int kFaMaxSplits = 256;

__global__ __launch_bounds__(256) void k_fa_combine(const fa_args a, int R, int DP) {
    __shared__ float w[kFaMaxSplits];
    __shared__ float red[256 / 64];
    const mi_fa_desc & d = a.d;
    const int r = blockIdx.x, blk = blockIdx.y;
    const int grp = blockIdx.z % a.ngrp, i3 = blockIdx.z / a.ngrp;
    const int row = blk * R + r;
    if (row >= d.N * a.G) return;  // workgroup-uniform
    const float * base = d.part + (((size_t) blockIdx.z * a.nblk + blk) * a.splits * R + r) * (DP + 2);
    const size_t stride = (size_t) R * (DP + 2);
    const int t = threadIdx.x;
    const float ms = t < a.splits ? base[t * stride + DP] : -INFINITY;
    const float wm = mi_wave_max(ms);
    if ((t & 63) == 0) red[t >> 6] = wm;
    __syncthreads();
    const float M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    w[t] = ms == -INFINITY ? 0.0f : fa_exp(ms - M);
    __syncthreads();
    if (t >= d.D) return;
    float L = 0.0f, O = 0.0f;
#pragma unroll 8
    for (int s = 0; s < a.splits; s++) {
        const float * p = base + s * stride;
        L += p[DP + 1] * w[s];
        O += p[t] * w[s];
    }
    int iq1, h;
    fa_row_of(a, grp, row, iq1, h);
    d.dst[(((size_t) i3 * d.N + iq1) * d.nh + h) * d.D + t] = O / L;
}

int fa_lpk(int D) { return D <= 64 ? 8 : D <= 128 ? 16 : 32; }

int fa_rows(const fa_args & a) {
    const int rtot = a.d.N * a.G;
    int R = 1;
    while (R < kFaMaxRows && R < rtot) R *= 2;
    return R;
}

fa_args fa_plan(const mi_fa_desc & d) {
    fa_args a;
    a.d = d;
    a.rk2 = d.nh / d.nh_k;
    a.rv2 = d.nh / d.nh_v;
    a.rk3 = d.ne3 / d.ne3_k;
    a.rv3 = d.ne3 / d.ne3_v;
    a.G = fa_gcd(a.rk2, a.rv2);
    a.ngrp = d.nh / a.G;
    a.mma = d.N >= kFaMmaMinN;
    const int R = fa_rows(a);
    a.nblk = (d.N * a.G + R - 1) / R;
    // enough workgroups for two per CU, each with at least kFaMinSplitKeys keys
    const int64_t wgs = (int64_t) a.ngrp * d.ne3 * a.nblk;
    int splits = (int) std::min<int64_t>((d.kv + kFaMinSplitKeys - 1) / kFaMinSplitKeys, std::max<int64_t>(1, kFaTargetWgs / wgs));
    splits = std::min(splits, kFaMaxSplits);
    splits = a.mma ? 1 : std::max(splits, 1);
    a.split_keys = ((d.kv + splits - 1) / splits + 15) & ~15;
    a.splits = std::max(1, (d.kv + a.split_keys - 1) / a.split_keys);
    a.n_head_log2 = 1;
    while (a.n_head_log2 * 2 <= d.nh) a.n_head_log2 *= 2;
    // src/ggml.c:15650-15654
    a.m0 = powf(2.0f, -(d.max_bias) / a.n_head_log2);
    a.m1 = powf(2.0f, -(d.max_bias / 2.0f) / a.n_head_log2);
    return a;
}

template <int R, int LPK>
void fa_launch_al(const fa_args & a, dim3 grid, bool al, hipStream_t s) {
    if (al) hipLaunchKernelGGL((k_fa_vec<R, LPK, true>), grid, dim3(64 * kFaWaves), 0, s, a);
    else hipLaunchKernelGGL((k_fa_vec<R, LPK, false>), grid, dim3(64 * kFaWaves), 0, s, a);
}

template <int R>
void fa_launch_lpk(const fa_args & a, dim3 grid, bool al, hipStream_t s) {
    switch (fa_lpk(a.d.D)) {
        case 8: fa_launch_al<R, 8>(a, grid, al, s); break;
        case 16: fa_launch_al<R, 16>(a, grid, al, s); break;
        default: fa_launch_al<R, 32>(a, grid, al, s); break;
    }
}

template <int DP, int KT>
void fa_launch_mma(const fa_args & a, bool al, hipStream_t s) {
    // 128 query rows per workgroup where that still gives every CU one, else 64
    const mi_fa_desc & d = a.d;
    const int nw = (int64_t) ((d.N + 127) / 128) * d.nh * d.ne3 >= 256 ? 4 : 2;
    const dim3 grid((unsigned) ((d.N + 32 * nw - 1) / (32 * nw)), (unsigned) d.nh, (unsigned) d.ne3);
    if (al) hipLaunchKernelGGL((k_fa_mma<DP, KT, true>), grid, dim3(64 * nw), 0, s, a);
    else hipLaunchKernelGGL((k_fa_mma<DP, KT, false>), grid, dim3(64 * nw), 0, s, a);
}

}  // namespace

bool mi_fa_head_size_ok(int64_t D) { return D == 64 || D == 80 || D == 96 || D == 112 || D == 128 || D == 256; }

int mi_fa_splits(const mi_fa_desc & d) { return fa_plan(d).splits; }

size_t mi_fa_part_bytes(const mi_fa_desc & d) {
    const fa_args a = fa_plan(d);
    if (a.splits == 1) return 0;
    return (size_t) a.ngrp * d.ne3 * a.nblk * a.splits * fa_rows(a) * (fa_lpk(d.D) * 8 + 2) * sizeof(float);
}

int mi_flash_attn_ext(const mi_fa_desc & d, hipStream_t s) {
    const fa_args a = fa_plan(d);
    // 16-byte loads need every K/V row on a 16-byte boundary
    const bool al = (((uintptr_t) d.k | (uintptr_t) d.v | d.nbk1 | d.nbk2 | d.nbk3 | d.nbv1 | d.nbv2 | d.nbv3) & 15) == 0;
    if (a.mma) {
        if (d.D <= 64) fa_launch_mma<64, 64>(a, al, s);
        else if (d.D <= 96) fa_launch_mma<96, 64>(a, al, s);
        else if (d.D <= 128) fa_launch_mma<128, 64>(a, al, s);
        else fa_launch_mma<256, 32>(a, al, s);
        return 1;
    }
    const int R = fa_rows(a);
    const dim3 grid((unsigned) a.splits, (unsigned) a.nblk, (unsigned) (a.ngrp * d.ne3));
    switch (R) {
        case 1: fa_launch_lpk<1>(a, grid, al, s); break;
        case 2: fa_launch_lpk<2>(a, grid, al, s); break;
        case 4: fa_launch_lpk<4>(a, grid, al, s); break;
        default: fa_launch_lpk<8>(a, grid, al, s); break;
    }
    if (a.splits == 1) return 1;
    hipLaunchKernelGGL(k_fa_combine, dim3((unsigned) R, (unsigned) a.nblk, (unsigned) (a.ngrp * d.ne3)), dim3(256), 0, s, a, R, fa_lpk(d.D) * 8);
    return 2;
}
