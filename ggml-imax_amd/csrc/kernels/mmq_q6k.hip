// mmq_q6k.hip -- batched (prompt / prefill) GGML_OP_MUL_MAT for Q6_K weights on the gfx950 int8
// matrix cores, with the reference's exact integer block sums.
//
// The reference dot product (ggml_vec_dot_q6_K_q8_K, src/ggml-quants.c:8730-9310) is, per superblock
// s of 256 weights of a row n and activation column b (Q8_K activations, no mins term),
//     y += d_a(b,s) * d_w(n,s) * T,   T = sum_{j<16} sc_j * D_j,   D_j = sum_{e<16} (q - 32)[16j + e] * a[16j + e]
// with q the 6-bit levels, sc_j the signed 8-bit scales of the sixteen 16-element sub-blocks. sc (q - 32)
// needs 14 bits, so the scale cannot ride in an int8 operand the way Q4_K's plane fields do (four
// planes, and a signed byte-wise multiply to build them). Instead the MFMA's K is the sub-block:
// v_mfma_i32_32x32x16_i8 from a zero accumulator is D_j of a 32 x 32 tile (|D_j| <= 16 * 32 * 128 =
// 2^16: a signed 24-bit operand), and T += sc_j * D_j is one v_mad_i32_i24 per accumulator register
// (|T| <= 2^27, exact int32). Per superblock t = fp16(d_w) * (float) T, and the terms are combined by
// the family's canonical fold (mmq_exact_common.h: g = fma(d_a, t, g) inside kCfoldGroups groups, the low
// and the high four group sums left-folded separately, y = lo + hi, + 0). Against the reference only
// that f32 order differs.
//
// Orientation: the weights are the MFMA's B operand, so the accumulator's N index (lane % 32) is the
// weight row: every accumulator register of a lane belongs to ONE row, and the sub-block's scale and
// d_w are one value per lane (the 16 scale bytes: 4 VGPRs, one v_bfe_i32 per sub-block). Lane (r, h =
// lane / 32) supplies elements 8h .. 8h + 7 of sub-block j of row r; its 16 registers are the prompt
// columns 8 (i / 4) + 4h + (i % 4), whose d_a are four float4 loads of xd; the stores dst[col][row] are
// 128-byte runs over r. (With the weights as A each lane would need the scales of 16 rows.)
//
// Decode (quant_decode.h: q6k_fmt, qd_q6k_levels): a "quarter" (hq, u) of a superblock is the dwords at
// p = 16u + 8h and p + 4 of ql[64 hq ..], ql[64 hq + 32 ..] and qh[32 hq ..]; two qd_q6k_levels calls turn
// them into the lane's two operand dwords of the four sub-blocks 8 hq + 2t + u (t = 0..3). Blocks are
// only 2-byte aligned (210 = 2 * 105) and rows of an odd superblock count are 2 mod 4, so every load
// is an aligned dword, re-aligned with v_alignbyte by the block's own misalignment (0 or 2, from its
// address): three dwords cover a lane's 8 bytes, five the 16 scales and d. The dword holding d may
// reach two bytes past the block (the next block, or the buffer's tail slack), as in the GEMV.
//
// Activations: the q8_K MFMA layout of mmq_exact.hip as it is (xq [K/32][ncols][32], xd; xu unused):
// the lane's 8 bytes of sub-block j are at 16 (j % 2) + 8h of 32-block j / 2.
//
// Two shapes of one template (k_mmq6<NT, STAGED>), bit-identical (the same terms, the same fold):
//   k_mmq6p  prompts of up to 64 columns, and any destination that is not local device memory: a 32 x 32 tile per
//            4-wave workgroup; wave w computes the canonical groups w and w + 4, the next superblock's
//            raw dwords requested before the current one's MFMAs; the group sums meet once in LDS.
//   k_mmq6x  long prompts: the workgroup (4 waves, 32 rows x 256 columns) stages the raw 210-byte blocks
//            of its rows for one superblock into LDS once (coalesced aligned dwords, double-buffered);
//            each wave decodes the rows once per superblock and uses every operand for its two
//            32-column tiles; it runs all eight groups itself (cfold_vec_park: the low half's sum waits
//            in LDS).

#include <algorithm>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#pragma clang fp contract(off)

#include "mmq_exact_common.h"
#include "quant_decode.h"

namespace {

using L6 = q6k_fmt;
constexpr int kQ6RowDw = 53;  // aligned dwords covering a block at either misalignment (2 + 210 = 4 * 53)

// block byte offset of a quarter's ql dwords for half h (lb: + 32) and of its qh dwords
__device__ __forceinline__ constexpr int q6_ql(int qi, int h) { return L6::QL + 64 * (qi >> 1) + 16 * (qi & 1) + 8 * h; }
__device__ __forceinline__ constexpr int q6_qh(int qi, int h) { return L6::QH + 32 * (qi >> 1) + 16 * (qi & 1) + 8 * h; }

// a lane's raw dwords of one superblock: per quarter the three aligned dwords covering its 8 bytes of
// ql[..], ql[.. + 32] and qh[..]; the five covering the 16 scales and d
struct Q6Raw {
    uint32_t q[4][9];
    uint32_t s[5];
};

// quarter qi's operands from its nine raw dwords: op[t][0..1] = the lane's 8 bytes of sub-block
// 8 (qi / 2) + 2t + (qi % 2) as q - 32
__device__ __forceinline__ void q6_quarter(const uint32_t (&w)[9], uint32_t off, int (&op)[4][2]) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t la = __builtin_amdgcn_alignbyte(w[i + 1], w[i], off);
        const uint32_t lb = __builtin_amdgcn_alignbyte(w[3 + i + 1], w[3 + i], off);
        const uint32_t hh = __builtin_amdgcn_alignbyte(w[6 + i + 1], w[6 + i], off);
        qd_q6k_levels<2>(la, lb, hh, &op[0][i]);
    }
}

// the 16 scale bytes as four dwords, and d
__device__ __forceinline__ float q6_scales(const uint32_t (&s)[5], uint32_t off, uint32_t (&sc)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) sc[i] = __builtin_amdgcn_alignbyte(s[i + 1], s[i], off);
    return mi_h2f((uint16_t) ((s[4] >> (8 * off)) & 0xFFFF));
}

// T += sc_j D_j for the four sub-blocks of quarter qi; xa[t]: the lane's column's 8 activation bytes
__device__ __forceinline__ void q6_mads(int (&T)[16], const int (&op)[4][2], const uint32_t (&sc)[4], const long (&xa)[4], int qi) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int j = 8 * (qi >> 1) + 2 * t + (qi & 1);
        const long b = (long) (((unsigned long) (uint32_t) op[t][1] << 32) | (uint32_t) op[t][0]);
        const i32x16 D = __builtin_amdgcn_mfma_i32_32x32x16_i8(xa[t], b, i32x16{}, 0, 0, 0);
        const int s = __builtin_amdgcn_sbfe(sc[j >> 2], 8 * (j & 3), 8);
#pragma unroll
        for (int e = 0; e < 16; e++) {
            T[e] += __mul24(s, D[e]);
            // (an opaque use: the integer sum is otherwise re-associated into a tree over the
            // sub-blocks, which keeps all their accumulators alive)
            asm volatile("" : "+v"(T[e]));
        }
        __builtin_amdgcn_sched_barrier(0);  // one sub-block's accumulator at a time
    }
}

template <int NT, bool STAGED>
__global__ __launch_bounds__(256, 2) void k_mmq6(mi_mmx_group grp) {
    MI_MMX_MEMBER(grp);
    constexpr int NW = 4;
    constexpr int TC = STAGED ? 32 * NT * NW : 32;  // columns per workgroup
    constexpr int kStage = 32 * kQ6RowDw;          // dwords of a staged superblock (32 rows)
    constexpr int kPasses = (kStage + 255) / 256;
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

    // The weights through a descriptor whose base is the tile's first row aligned down to a dword; a
    // block's dwords are then at voff (lane: row offset, minus the block's misalignment) + soff (the
    // superblock, a multiple of 4: 210 sb - 2 (sb & 1), the other 2 bytes of an odd one in voff).
    const uint8_t * wt = W + n0 * nb01;
    const uint32_t bmis = (uint32_t) (uintptr_t) wt & 2;
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void *) (wt - bmis), (short) 0, (int) (bmis + nrows * nb01 + 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xq, (short) 0, (int) (K * ncols), 0x00020000);
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xd, (short) 0, (int) (S * ncols * 4), 0x00020000);
    auto row_off = [&](int row) { return bmis + (uint32_t) (std::min(row, nrows - 1) * nb01); };
    auto sb_soff = [](int sb) { return (uint32_t) __builtin_amdgcn_readfirstlane(sb * L6::BS - 2 * (sb & 1)); };
    // this lane's row: its offset, its blocks' misalignment in an even superblock (an odd one: the other)
    const uint32_t wrow = row_off(r);
    const uint32_t rmis = wrow & 2;
    auto blk_mis = [&](int sb) { return rmis ^ (uint32_t) (2 * (sb & 1)); };

    const uint32_t xstep = (uint32_t) ncols * 32;
    // activations of quarter qi of superblock sb for the tile at column cb: 8 bytes of 32-blocks 4 (qi / 2) + t
    auto load_xa = [&](long (&xa)[4], int sb, int qi, uint32_t acol) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t so = (uint32_t) __builtin_amdgcn_readfirstlane((sb * 8 + 4 * (qi >> 1) + t) * (int) xstep);
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(xres, acol * 32 + 16 * (qi & 1) + 8 * h, so, 0);
            xa[t] = __builtin_bit_cast(long, v);
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
        auto load_raw = [&](Q6Raw & o, int sb) {
            const uint32_t so = sb_soff(sb);
            const uint32_t vo = wrow - blk_mis(sb) + 2 * (sb & 1);
#pragma unroll
            for (int qi = 0; qi < 4; qi++)
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    // (h is folded into the lane offset: the immediate part stays a constant)
                    o.q[qi][i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + q6_ql(qi, 0) + 4 * i, so, 0);
                    o.q[qi][3 + i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + q6_ql(qi, 0) + 32 + 4 * i, so, 0);
                    o.q[qi][6 + i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + q6_qh(qi, 0) + 4 * i, so, 0);
                }
#pragma unroll
            for (int i = 0; i < 5; i++) o.s[i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + L6::SC + 4 * i, so, 0);
        };
        f32x16 gsum = {};
        if (nsb > 0) {
            Q6Raw raw[2];
            long xa[2][4];
            load_raw(raw[0], sb_at(0));
            load_xa(xa[0], sb_at(0), 0, acol);
            float dan = ld_d(sb_at(0), acol);
            // the wave's k-th superblock from `cur`; superblock k + 1's raw dwords go into `nxt`, each
            // quarter's activations are requested a quarter ahead
            auto step = [&](const Q6Raw & cur, Q6Raw & nxt, const int k) {
                const int sb = sb_at(k), sn = sb_at(k + 1);
                const bool first = sb % gs == 0, last = sb % gs == gs - 1 || sb == S - 1;
                load_raw(nxt, sn);
                const uint32_t off = blk_mis(sb);
                uint32_t sc[4];
                const float dw = q6_scales(cur.s, off, sc);
                const float dac = dan;
                dan = ld_d(sn, acol);
                int T[16] = {};
#pragma unroll
                for (int qi = 0; qi < 4; qi++) {
                    if (qi < 3) load_xa(xa[(qi + 1) & 1], sb, qi + 1, acol);
                    else load_xa(xa[0], sn, 0, acol);
                    int op[4][2];
                    q6_quarter(cur.q[qi], off, op);
                    q6_mads(T, op, sc, xa[qi & 1], qi);
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
        // staging role: dword i = tid + 256 k of the stage = dword i % 53 of row i / 53
        float * parked = (float *) (lds + 2 * kStage) + w * NT * 16 * 64;
        uint32_t svo[kPasses];   // voff of an even superblock
        uint32_t sodd = 0;       // bit k: the row is misaligned (an odd superblock's dwords lie 4 bytes on)
#pragma unroll
        for (int k = 0; k < kPasses; k++) {
            const int i = std::min(tid + 256 * k, kStage - 1);
            const int row = i / kQ6RowDw, dw = i - row * kQ6RowDw;
            const uint32_t ro = row_off(row);
            svo[k] = ro - (ro & 2) + 4 * dw;
            sodd |= ((ro >> 1) & 1) << k;
        }
        auto load_stage = [&](uint32_t (&st)[kPasses], int sb) {
            sb = sb < S ? sb : S - 1;
            const uint32_t so = sb_soff(sb);
            const uint32_t odd = (sb & 1) ? sodd : 0;
#pragma unroll
            for (int k = 0; k < kPasses; k++)
                st[k] = __builtin_amdgcn_raw_buffer_load_b32(wres, svo[k] + (((odd >> k) & 1) << 2), so, 0);
        };
        auto store_stage = [&](const uint32_t (&st)[kPasses], int buf) {
#pragma unroll
            for (int k = 0; k < kPasses; k++)
                if (tid + 256 * k < kStage) lds[buf * kStage + tid + 256 * k] = st[k];
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
        long xa[2][NT][4];
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
            const uint32_t * blk = lds + (sb & 1) * kStage + r * kQ6RowDw;
            const int sn = sb + 1 < S ? sb + 1 : S - 1;
            const uint32_t off = blk_mis(sb);
            uint32_t sw[5], sc[4];
#pragma unroll
            for (int i = 0; i < 5; i++) sw[i] = blk[L6::SC / 4 + i];
            const float dw = q6_scales(sw, off, sc);
            int T[NT][16] = {};
#pragma unroll
            for (int qi = 0; qi < 4; qi++) {
#pragma unroll
                for (int ct = 0; ct < NT; ct++) {
                    if (qi < 3) load_xa(xa[(qi + 1) & 1][ct], sb, qi + 1, acol[ct]);
                    else load_xa(xa[0][ct], sn, 0, acol[ct]);
                }
                uint32_t wq[9];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    wq[i] = blk[q6_ql(qi, 0) / 4 + 2 * h + i];
                    wq[3 + i] = blk[q6_ql(qi, 0) / 4 + 8 + 2 * h + i];
                    wq[6 + i] = blk[q6_qh(qi, 0) / 4 + 2 * h + i];
                }
                int op[4][2];
                q6_quarter(wq, off, op);
#pragma unroll
                for (int ct = 0; ct < NT; ct++) q6_mads(T[ct], op, sc, xa[qi & 1][ct], qi);
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

// Q6_K (q8_K activations). Prompts of up to 64 columns, and every destination that is not local
// device memory: k_mmq6p; longer ones: k_mmq6x, whose 256-column tiles cost the same from 65 to 256
// columns (profiles/q6k_prefill.txt, us per mul_mat, k_mmq6p / k_mmq6x: 4096 x 4096 B = 64 22.2 / 20.7,
// B = 128 41.7 / 21.2; 11008 x 4096 B = 64 45.3 / 50.8, B = 128 84.1 / 52.4: the shapes disagree at 64,
// k_mmq6x wins by 1.6-2x at 128). kMmqShortKernels / kMmqLongKernels force either at any column count.
// Both follow the canonical combine order: the same bits.
void mi_mmq6_group(mi_mmx_group & g, hipStream_t s, bool dst_local) {
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
    if ((var & kMmqShortKernels) || (ncols <= 64 && !(var & kMmqLongKernels)) || !dst_local) {
        mi_route("k_mmq6p");
        hipLaunchKernelGGL((k_mmq6<1, false>), dim3((unsigned) deal(32)), dim3(256), 0, s, g);
        return;
    }
    mi_route("k_mmq6x");
    hipLaunchKernelGGL((k_mmq6<2, true>), dim3((unsigned) deal(256)), dim3(256), 0, s, g);
}
