// mmq_iq4xs.hip -- batched (prompt / prefill) GGML_OP_MUL_MAT for IQ4_XS weights on the gfx950 int8
// matrix cores, with the reference's exact integer block sums.
//
// The reference dot product (ggml_vec_dot_iq4_xs_q8_K, src/ggml-quants.c:11873-11967) is, per superblock
// s of 256 weights of a row n and activation column b (Q8_K activations),
//     y += d_a(b,s) * d_w(n,s) * T,   T = sum_{ib<8} (ls_ib - 32) * D_ib,   D_ib = sum_{e<32} kvalues[q[32 ib + e]] * a[32 ib + e]
// with q the 4-bit codebook indices, kvalues the int8 levels kvalues_iq4nl (-127 .. 113) and ls_ib the
// 6-bit scales of the eight 32-element sub-blocks. A sub-block is exactly the K of
// v_mfma_i32_32x32x32_i8: one MFMA from a zero accumulator is D_ib of a 32 x 32 tile (|D_ib| <= 32 * 127 *
// 128 = 520 192 < 2^23: a signed 24-bit operand), and T += (ls_ib - 32) * D_ib is one v_mad_i32_i24 per
// accumulator register (|T| <= 8 * 32 * 520 192 < 2^27, exact int32): half the MFMAs and half the mads
// per superblock of Q6_K's kernel (mmq_q6k.hip), whose sub-blocks are 16 elements. Per superblock t =
// fp16(d_w) * (float) T, and the terms are combined by the family's canonical fold
// (mmq_exact_common.h: g = fma(d_a, t, g) inside kCfoldGroups groups, the low and the high four group
// sums left-folded separately, y = lo + hi, + 0). Against the reference only that f32 order differs.
//
// Orientation (as k_mmq6): the weights are the MFMA's B operand, so the accumulator's N index (lane %
// 32) is the weight row: every accumulator register of a lane belongs to ONE row, and the sub-block's
// scale and d_w are one value per lane (qd_iq4xs_scale on the block's first two dwords: d | scales_h
// and scales_l). The lane's 16 registers are the prompt columns 8 (i / 4) + 4h + (i % 4), whose d_a
// reach it through a wave-private LDS row; the stores dst[col][row] are 128-byte runs over r.
//
// Decode: the nibble layout is the lane halves'. Element j < 16 of sub-block ib is the low nibble of
// qs[16 ib + j], element 16 + j the high one: lane (r, h = lane / 32) takes the 16 qs bytes of its
// row's sub-block (four dwords: blocks are 136 bytes = 34 dwords of rows that start on a dword, so
// nothing is re-aligned), and mi_iq4nl_levels(w >> 4h) (three v_perm_b32 per four weights; it masks
// the other nibbles off itself) makes them its 16-byte operand, elements 16h .. 16h + 15. No nibble is
// decoded twice.
//
// Activations: the q8_K MFMA layout of mmq_exact.hip as it is (xq [K/32][ncols][32], xd; xu unused):
// the lane's column's elements 16h .. 16h + 15 of sub-block ib are the 16 bytes at 16h of 32-block 8 sb
// + ib, one b128 buffer load. Both operands give element 16h + i to lane half h, byte i, so the integer
// sum is right whatever K slot the hardware assigns to (h, i).
//
// Two shapes of one template (k_mmqi4<NT, STAGED>), bit-identical (the same terms, the same fold):
//   k_mmqi4p  short prompts, and any destination that is not local device memory: a 32 x 32 tile per
//             4-wave workgroup; wave w computes the canonical groups w and w + 4, the next superblock's
//             raw dwords requested before the current one's MFMAs; the group sums meet once in LDS.
//   k_mmqi4x  long prompts: the workgroup (4 waves, 32 rows x 256 columns) stages the 34 dwords of its
//             rows for one superblock into LDS once (coalesced dwords, double-buffered; a row takes 36
//             dwords there, the block from the third on, so its quants are 16-byte aligned); each wave
//             decodes a row's sub-block once and uses the operand for its two 32-column tiles; it runs
//             all eight groups itself (cfold_vec_park: the low half's sum waits in LDS).

#include <algorithm>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#pragma clang fp contract(off)

#include "mmq_exact_common.h"
#include "quant_decode.h"

namespace {

constexpr int kI4BS = mi_type(MI_TYPE_IQ4_XS).bytes;  // 136
constexpr int kI4Dw = kI4BS / 4;                      // dwords of a block
constexpr int kI4Row = kI4Dw + 2;                     // dwords of a staged row: two of padding, then the block
static_assert(kI4BS % 4 == 0 && (kI4Row * 4) % 16 == 0, "IQ4_XS blocks are whole dwords; staged quants 16-byte aligned");

// a lane's raw dwords of one superblock: the header (d | scales_h << 16, scales_l) and the 16 quant
// bytes of each of the row's eight sub-blocks
struct I4Raw {
    uint32_t hd, sl;
    uint4 q[8];
};

// the lane's operand of a sub-block from its 16 quant bytes: the levels of the low (h = 0: sh 0) or
// the high (sh 4) nibbles
__device__ __forceinline__ i32x4 i4_operand(const uint4 & w, int sh) {
    return i32x4{mi_iq4nl_levels(w.x >> sh), mi_iq4nl_levels(w.y >> sh), mi_iq4nl_levels(w.z >> sh), mi_iq4nl_levels(w.w >> sh)};
}

// T += (ls_ib - 32) D_ib; xa: the lane's column's 16 activation bytes, b: the row's operand
__device__ __forceinline__ void i4_mad(int (&T)[16], const i32x4 & xa, const i32x4 & b, int s) {
    const i32x16 D = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, b, i32x16{}, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        T[e] += __mul24(s, D[e]);
        // (an opaque use: the integer sum is otherwise re-associated into a tree over the
        // sub-blocks, which keeps all their accumulators alive)
        asm volatile("" : "+v"(T[e]));
    }
    __builtin_amdgcn_sched_barrier(0);  // one sub-block's accumulator at a time
}

template <int NT, bool STAGED>
__global__ __launch_bounds__(256, 2) void k_mmqi4(mi_mmx_group grp) {
    MI_MMX_MEMBER(grp);
    constexpr int NW = 4;
    constexpr int TC = STAGED ? 32 * NT * NW : 32;  // columns per workgroup
    constexpr int kLoad = 32 * kI4Dw;               // dwords of a superblock of 32 rows
    constexpr int kStage = 32 * kI4Row;             // ... and of its stage buffer
    constexpr int kPasses = (kLoad + 255) / 256;
    // STAGED: two stage buffers and the parked low halves [wave][tile][el][lane]; else the group sums
    // [group][el][lane]
    __shared__ __attribute__((aligned(16))) uint32_t lds[STAGED ? 2 * kStage + NW * NT * 16 * 64 : kCfoldGroups * 16 * 64];
    __shared__ __attribute__((aligned(16))) float dal[NW][NT][32];  // per-wave d_a rows
    const int tid = (int) threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int64_t ncols = act.ncols;
    const int S = (int) (K / 256);
    const int gs = cfold_gs(S);
    const int64_t nrt = (N + 31) / 32;
    const int64_t n0 = (mmx_tile % nrt) * 32, c0 = (mmx_tile / nrt) * TC + (STAGED ? 32 * NT * w : 0);
    const int nrows = (int) std::min<int64_t>(32, N - n0);

    // The tile's rows, the activations and their scales through descriptors of exactly their bytes:
    // rows past the tile's last and columns past the prompt's last are clamped to the last one (their
    // results are not stored), so every load lies inside.
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void *) (W + n0 * nb01), (short) 0, (int) (nrows * nb01), 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xq, (short) 0, (int) (K * ncols), 0x00020000);
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xd, (short) 0, (int) (S * ncols * 4), 0x00020000);
    auto row_off = [&](int row) { return (uint32_t) (std::min(row, nrows - 1) * nb01); };
    auto sb_soff = [](int sb) { return (uint32_t) __builtin_amdgcn_readfirstlane(sb * kI4BS); };
    const int nsh = 4 * h;  // the lane half's nibble

    const uint32_t xstep = (uint32_t) ncols * 32;
    // the column's 16 activation bytes of sub-blocks 4 hf .. 4 hf + 3 of superblock sb
    auto load_xa = [&](i32x4 (&xa)[4], int sb, int hf, uint32_t acol) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t so = (uint32_t) __builtin_amdgcn_readfirstlane((sb * 8 + 4 * hf + t) * (int) xstep);
            xa[t] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(xres, acol * 32 + 16 * h, so, 0));
        }
    };
    // d_a: each lane loads its own (clamped) column's, a superblock ahead; the lane's 16 columns' reach
    // it through a wave-private LDS row as four float4 (a direct float4 load of xd would run past
    // the last superblock's row in a ragged column tile)
    auto ld_d = [&](int sb, uint32_t acol) {
        const uint32_t so = (uint32_t) __builtin_amdgcn_readfirstlane(sb * (int) ncols * 4);
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dres, acol * 4, so, 0));
    };
    auto spread_da = [&](f32x16 & da, float mine, float * row) {
        if (h == 0) row[r] = mine;
        __builtin_amdgcn_wave_barrier();
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 d4 = *(const float4 *) &row[8 * g + 4 * h];
            da[4 * g] = d4.x; da[4 * g + 1] = d4.y; da[4 * g + 2] = d4.z; da[4 * g + 3] = d4.w;
        }
        __builtin_amdgcn_wave_barrier();  // the row is rewritten by the next superblock
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
    };
    // the lane's outputs of the tile at column cb: row n0 + r, columns cb + 8 (el / 4) + 4h + (el % 4)
    auto store_tile = [&](const f32x16 & y, int64_t cb) {
        if (r >= nrows) return;
#pragma unroll
        for (int el = 0; el < 16; el++) {
            const int64_t c = cb + 8 * (el >> 2) + 4 * h + (el & 3);
            if (c < ncols) *(float *) ((char *) dst + c * ycol + (n0 + r) * sizeof(float)) = y[el];
        }
    };

    if constexpr (!STAGED) {
        constexpr int NG = kCfoldGroups / NW;
        float * red = (float *) lds;
        auto gbeg = [&](int i) { return min(S, (w + NW * i) * gs); };
        auto gend = [&](int i) { return min(S, (w + NW * i + 1) * gs); };
        const int nsb = [&] { int n = 0; for (int i = 0; i < NG; i++) n += gend(i) - gbeg(i); return n; }();
        // the wave's k-th superblock (clamped to its last one)
        auto sb_at = [&](int k) {
            k = min(k, nsb - 1);
#pragma unroll
            for (int i = 0; i < NG; i++) {
                const int len = gend(i) - gbeg(i);
                if (k < len) return gbeg(i) + k;
                k -= len;
            }
            return S - 1;
        };
        const uint32_t acol = (uint32_t) std::min<int64_t>(c0 + r, ncols - 1);
        const uint32_t wrow = row_off(r);
        auto load_raw = [&](I4Raw & o, int sb) {
            const uint32_t so = sb_soff(sb);
            o.hd = __builtin_amdgcn_raw_buffer_load_b32(wres, wrow, so, 0);
            o.sl = __builtin_amdgcn_raw_buffer_load_b32(wres, wrow + 4, so, 0);
#pragma unroll
            for (int ib = 0; ib < 8; ib++)
                o.q[ib] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wres, wrow + 8 + 16 * ib, so, 0));
        };
        f32x16 gsum = {};
        if (nsb > 0) {
            I4Raw raw[2];
            i32x4 xa[2][4];
            load_raw(raw[0], sb_at(0));
            load_xa(xa[0], sb_at(0), 0, acol);
            float dan = ld_d(sb_at(0), acol);
            // the wave's k-th superblock from `cur`; superblock k + 1's raw dwords go into `nxt`, each
            // half's activations are requested a half ahead
            auto step = [&](const I4Raw & cur, I4Raw & nxt, const int k) {
                const int sb = sb_at(k), sn = sb_at(k + 1);
                const bool first = sb % gs == 0, last = sb % gs == gs - 1 || sb == S - 1;
                load_raw(nxt, sn);
                const float dw = mi_h2f((uint16_t) (cur.hd & 0xFFFF));
                const float dac = dan;
                dan = ld_d(sn, acol);
                int T[16] = {};
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    if (hf == 0) load_xa(xa[1], sb, 1, acol);
                    else load_xa(xa[0], sn, 0, acol);
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int ib = 4 * hf + t;
                        i4_mad(T, xa[hf][t], i4_operand(cur.q[ib], nsh), qd_iq4xs_scale(cur.sl, cur.hd >> 16, ib));
                    }
                }
                f32x16 da;
                spread_da(da, dac, dal[w][0]);
                if (first) {  // uniform: a group starts at -0 (-0 + t == t), kept a branch (no selects)
                    asm volatile("" ::: "memory");
                    gsum = f32x16(-0.0f);
                }
#pragma unroll
                for (int el = 0; el < 16; el++) gsum[el] = __builtin_fmaf(da[el], dw * (float) T[el], gsum[el]);
                if (last) {  // the group's sum -> LDS slot of group sb / gs
                    const int gi = sb / gs;
#pragma unroll
                    for (int el = 0; el < 16; el++) red[(gi * 16 + el) * 64 + lane] = gsum[el];
                }
            };
            for (int k = 0; k < nsb; k += 2) {
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (k + u >= nsb) break;
                    step(raw[u], raw[u ^ 1], k + u);
                }
            }
        }
        mi_lds_barrier();
        // the group sums folded (canonical order) by the whole workgroup: output o = el 64 + l -- lanes
        // 0..31 store 32 consecutive rows
        const int ngroups = (S + gs - 1) / gs;
#pragma unroll
        for (int i = 0; i < 16 / NW; i++) {
            const int o = tid + 64 * NW * i;
            const int el = o >> 6, l = o & 63;
            const float y = cfold_groups(ngroups, [&](int v) { return red[(v * 16 + el) * 64 + l]; });
            const int64_t n = n0 + (l & 31);
            const int64_t c = c0 + (el & 3) + 8 * (el >> 2) + 4 * (l >> 5);
            if (n < N && c < ncols) *(float *) ((char *) dst + c * ycol + n * sizeof(float)) = y;
        }
    } else {
        // staging role: dword i = tid + 256 k of the superblock's 32 x 34 = dword i % 34 of row i / 34,
        // kept at dword 2 + i % 34 of the row's 36 in LDS
        float * parked = (float *) (lds + 2 * kStage) + w * NT * 16 * 64;
        uint32_t svo[kPasses];  // its byte offset in the tile's rows
        int sls[kPasses];       // its dword in a stage buffer
#pragma unroll
        for (int k = 0; k < kPasses; k++) {
            const int i = std::min(tid + 256 * k, kLoad - 1);
            const int row = i / kI4Dw, dw = i - row * kI4Dw;
            svo[k] = row_off(row) + 4 * dw;
            sls[k] = row * kI4Row + 2 + dw;
        }
        auto load_stage = [&](uint32_t (&st)[kPasses], int sb) {
            sb = sb < S ? sb : S - 1;
            const uint32_t so = sb_soff(sb);
#pragma unroll
            for (int k = 0; k < kPasses; k++) st[k] = __builtin_amdgcn_raw_buffer_load_b32(wres, svo[k], so, 0);
        };
        auto store_stage = [&](const uint32_t (&st)[kPasses], int buf) {
#pragma unroll
            for (int k = 0; k < kPasses; k++)
                if (tid + 256 * k < kLoad) lds[buf * kStage + sls[k]] = st[k];
        };
        uint32_t acol[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) acol[ct] = (uint32_t) std::min<int64_t>(c0 + 32 * ct + r, ncols - 1);

        f32x16 y[NT], gsum[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) {
            y[ct] = f32x16(-0.0f);  // cfold_vec_park's first group sum lands exactly
            gsum[ct] = f32x16{};
        }
        uint32_t st[kPasses];
        i32x4 xa[2][NT][4];
        load_stage(st, 0);
        store_stage(st, 0);
        load_stage(st, 1);
#pragma unroll
        for (int ct = 0; ct < NT; ct++) load_xa(xa[0][ct], 0, 0, acol[ct]);
        float dan[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) dan[ct] = ld_d(0, acol[ct]);
        mi_lds_barrier();
        for (int sb = 0; sb < S; sb++) {
            const uint32_t * blk = lds + (sb & 1) * kStage + r * kI4Row + 2;
            const int sn = sb + 1 < S ? sb + 1 : S - 1;
            const uint2 hdr = *(const uint2 *) blk;  // d | scales_h << 16, scales_l
            const float dw = mi_h2f((uint16_t) (hdr.x & 0xFFFF));
            int T[NT][16] = {};
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
#pragma unroll
                for (int ct = 0; ct < NT; ct++) {
                    if (hf == 0) load_xa(xa[1][ct], sb, 1, acol[ct]);
                    else load_xa(xa[0][ct], sn, 0, acol[ct]);
                }
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int ib = 4 * hf + t;
                    const i32x4 b = i4_operand(*(const uint4 *) (blk + 2 + 4 * ib), nsh);
                    const int s = qd_iq4xs_scale(hdr.y, hdr.x >> 16, ib);
#pragma unroll
                    for (int ct = 0; ct < NT; ct++) i4_mad(T[ct], xa[hf][ct][t], b, s);
                }
            }
            // the stage's successor into the other buffer (its readers passed the last barrier), then
            // the request for the one after
            store_stage(st, (sb + 1) & 1);
            load_stage(st, sb + 2);
#pragma unroll
            for (int ct = 0; ct < NT; ct++) {
                f32x16 da, tv;
                spread_da(da, dan[ct], dal[w][ct]);
                dan[ct] = ld_d(sn, acol[ct]);
#pragma unroll
                for (int el = 0; el < 16; el++) tv[el] = dw * (float) T[ct][el];
                float * pk = parked + ct * 16 * 64 + lane;
                cfold_vec_park(gsum[ct], y[ct], tv, da, sb, gs, S, [&](const f32x16 & v) {
#pragma unroll
                    for (int el = 0; el < 16; el++) pk[el * 64] = v[el];
                });
            }
            mi_lds_barrier();
        }
#pragma unroll
        for (int ct = 0; ct < NT; ct++) {
            if (cfold_split(S) < S) {  // cfold_end: the parked low half + the high half
                const float * pk = parked + ct * 16 * 64 + lane;
                f32x16 lo;
#pragma unroll
                for (int el = 0; el < 16; el++) lo[el] = pk[el * 64];
                y[ct] = lo + y[ct];
            }
            store_tile(cfold_pos_zero_vec(y[ct]), c0 + 32 * ct);
        }
    }
}

} // namespace

// IQ4_XS (q8_K activations). Prompts of up to 128 columns, and every destination that is not local
// device memory: k_mmqi4p; longer ones: k_mmqi4x, whose 256-column tiles cost the same from 9 to 256
// columns (profiles/iq4xs_prefill.txt, us per mul_mat, k_mmqi4p / k_mmqi4x: 4096 x 4096 B = 64 9.4 / 15.6,
// B = 128 16.9 / 15.9, B = 512 62.3 / 32.1; 11008 x 4096 B = 64 18.4 / 37.6, B = 128 33.9 / 38.1, B = 512
// 127.1 / 77.9: k_mmqi4p wins by 1.7-2x at 64, the shapes disagree at 128, k_mmqi4x wins by 1.6-2x at
// 512). kMmqShortKernels / kMmqLongKernels force either at any column count. Both follow the canonical
// combine order: the same bits.
void mi_mmqi4_group(mi_mmx_group & g, hipStream_t s, bool dst_local) {
    const int var = g_mi_tuning.mmq_variant;
    const int64_t ncols = g.m[0].act.ncols;
    auto deal = [&](int64_t tc) {
        int64_t t = 0;
        for (int i = 0; i < g.n; i++) {
            g.m[i].tile_begin = t;
            t += ((g.m[i].N + 31) / 32) * ((g.m[i].act.ncols + tc - 1) / tc);
        }
        return t;
    };
    if ((var & kMmqShortKernels) || (ncols <= 128 && !(var & kMmqLongKernels)) || !dst_local) {
        mi_route("k_mmqi4p");
        hipLaunchKernelGGL((k_mmqi4<1, false>), dim3((unsigned) deal(32)), dim3(256), 0, s, g);
        return;
    }
    mi_route("k_mmqi4x");
    hipLaunchKernelGGL((k_mmqi4<2, true>), dim3((unsigned) deal(256)), dim3(256), 0, s, g);
}
