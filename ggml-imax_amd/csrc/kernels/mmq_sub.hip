// mmq_sub.hip -- batched (prompt / prefill) GGML_OP_MUL_MAT on the gfx950 int8 matrix cores with the
// reference's exact integer block sums, one MFMA per sub-block: Q6_K (sub_q6k), IQ4_XS (sub_iq4xs), Q3_K
// (sub_q3k) and Q2_K (sub_q2k).
//
// The reference dot products are, per superblock s of 256 weights of a row n and activation column b
// (Q8_K activations),
//     y += d_a(b,s) * d_w(n,s) * T,   T = sum_j s_j * D_j,   D_j = sum_e level[j][e] * a[j][e]
// with s_j the signed scale of sub-block j; Q2_K alone has a mins term, y -= d_a dmin_w U with U = sum_j
// m_j bsum_j, which its policy computes exactly from the activation bytes in hand and two more MFMAs per
// superblock (sub_q23k), t = fma(-dmin_w, U, d_w T) (mmqx_pre). s_j level does not fit an int8 operand the way Q4_K's plane
// fields do, so the MFMA's K is the sub-block: one MFMA from a zero accumulator is D_j of a 32 x 32 tile
// (a signed 24-bit operand), and T += s_j * D_j is one v_mad_i32_i24 per accumulator register (exact
// int32; the bounds are with each format). Per superblock t = fp16(d_w) * (float) T, and the terms are
// combined by the family's canonical fold (mmq_exact_common.h: g = fma(d_a, t, g) inside kCfoldGroups
// groups, the low and the high four group sums left-folded separately, y = lo + hi, + 0). Against the
// reference only that f32 order differs.
//
// Orientation: the weights are the MFMA's B operand, so the accumulator's N index (lane % 32) is the
// weight row: every accumulator register of a lane belongs to ONE row, and the sub-block's scale and
// d_w are one value per lane. Lane (r, h = lane / 32) supplies half h of the elements of sub-block j of
// row r; its 16 registers are the prompt columns 8 (i / 4) + 4h + (i % 4), whose d_a reach it through a
// wave-private LDS row as four float4; the stores dst[col][row] are 128-byte runs over r. (With the
// weights as A each lane would need the scales of 16 rows.)
//
// Activations: the q8_K MFMA layout of mmq_exact.hip as it is (xq [K/32][ncols][32], xd; xu unused).
// Both operands give the same element to lane half h, byte i, so the integer sum is right whatever K
// slot the hardware assigns to (h, i).
//
// A format F gives: its block's raw dwords (from memory into a lane's registers, or read from the
// row's dwords in a stage buffer), d_w and the scales from them (Head; Q2_K: dmin and the mins too), one
// phase of the superblock -- four sub-blocks, whose activations are requested a phase ahead -- any state
// the phases leave for a mins term (Mins, mins_term; empty but for Q2_K) and the superblock's t (term).
//
// Two shapes of one template (k_mmqs<F, NT, STAGED>), bit-identical (the same terms, the same fold):
//   short  (k_mmq6p, k_mmqi4p, k_mmq3p, k_mmq2p) short prompts, and any destination that is not local device memory: a
//          32 x 32 tile per 4-wave workgroup; wave w computes the canonical groups w and w + 4, the next
//          superblock's raw dwords requested before the current one's MFMAs; the group sums meet once
//          in LDS.
//   long   (k_mmq6x, k_mmqi4x, k_mmq3x, k_mmq2x) long prompts: the workgroup (4 waves, 32 rows x 256 columns) stages the
//          raw blocks of its rows for one superblock into LDS once (coalesced aligned dwords,
//          double-buffered); each wave decodes the rows once per superblock and uses every operand for
//          its two 32-column tiles; it runs all eight groups itself (cfold_vec_park: the low half's sum
//          waits in LDS).

#include <algorithm>
#include <type_traits>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#pragma clang fp contract(off)

#include "mmq_exact_common.h"
#include "quant_decode.h"

namespace {

// T += s D for one sub-block; xa: the lane's column's activation bytes, b: the row's operand
template <typename F>
__device__ __forceinline__ void sub_mad(int (&T)[16], const typename F::Op & xa, const typename F::Op & b, int s) {
    const i32x16 D = F::mfma(xa, b);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        T[e] += __mul24(s, D[e]);
        // (an opaque use: the integer sum is otherwise re-associated into a tree over the
        // sub-blocks, which keeps all their accumulators alive)
        asm volatile("" : "+v"(T[e]));
    }
    __builtin_amdgcn_sched_barrier(0);  // one sub-block's accumulator at a time
}

// A format without a mins term: no state through the phases, t = d_w T
struct sub_no_mins {
    template <int NT> struct Mins {};
    struct NoU {};
    template <typename M, typename H> static __device__ __forceinline__ NoU mins_term(const M &, const H &, int) { return {}; }
    template <typename H> static __device__ __forceinline__ float term(int T, NoU, int, float dw, const H &) { return dw * (float) T; }
};

// Q6_K. Reference: ggml_vec_dot_q6_K_q8_K (src/ggml-quants.c:8730-9310): D_j = sum_{e<16} (q - 32)[16j + e]
// a[16j + e] with q the 6-bit levels and sc_j the signed 8-bit scales of the sixteen 16-element
// sub-blocks (sc (q - 32) needs 14 bits). v_mfma_i32_32x32x16_i8: |D_j| <= 16 * 32 * 128 = 2^16, |T| <=
// 2^27. The 16 scale bytes are 4 VGPRs, one v_bfe_i32 per sub-block.
//
// Decode (quant_decode.h: q6k_fmt, qd_q6k_levels): a phase is a "quarter" (hq = qi / 2, u = qi % 2) of a
// superblock: the dwords at p = 16u + 8h and p + 4 of ql[64 hq ..], ql[64 hq + 32 ..] and qh[32 hq ..];
// two qd_q6k_levels calls turn them into the lane's two operand dwords (elements 8h .. 8h + 7) of the
// four sub-blocks 8 hq + 2t + u (t = 0..3), whose 8 activation bytes are at 16u + 8h of 32-block 4 hq + t.
// Blocks are only 2-byte aligned (210 = 2 * 105) and rows of an odd superblock count are 2 mod 4, so
// every load is an aligned dword, re-aligned with v_alignbyte by the block's own misalignment (0 or 2,
// from its address): three dwords cover a lane's 8 bytes, five the 16 scales and d. The dword holding
// d may reach two bytes past the block (the next block, or the buffer's tail slack), as in the GEMV.
struct sub_q6k : sub_no_mins {
    using L = q6k_fmt;
    using Op = long;
    static constexpr int BS = L::BS;
    static constexpr int kPhases = 4;
    static constexpr int kSlack = 4;     // the dword holding the last block's d
    static constexpr int kLoadDw = 53;   // aligned dwords covering a block at either misalignment (2 + 210 = 4 * 53)
    static constexpr int kRowDw = 53, kBlkDw = 0;  // a staged row: those dwords
    // Prompts of up to 64 columns: k_mmq6p; longer ones: k_mmq6x, whose 256-column tiles cost the same
    // from 65 to 256 columns (profiles/q6k_prefill.txt, us per mul_mat, k_mmq6p / k_mmq6x: 4096 x 4096 B =
    // 64 22.2 / 20.7, B = 128 41.7 / 21.2; 11008 x 4096 B = 64 45.3 / 50.8, B = 128 84.1 / 52.4: the shapes
    // disagree at 64, k_mmq6x wins by 1.6-2x at 128). Those are the figures the crossover was chosen on. In this
    // file's build the short shape's 36 three-dword raw loads per superblock are all merged (dwordx3; the
    // build of the file this came from kept 24 of them as single dwords in the loop) and k_mmq6p takes
    // 0.5-0.6 of those times (profiles/mmq_sub_ab.txt: 4096 x 4096 B = 64 11.3 / 20.6, B = 128 20.3 / 20.6;
    // 11008 x 4096 B = 64 26.9 / 49.7, B = 128 48.8 / 50.9): level at 128. The crossover is not moved on that.
    static constexpr int64_t kShortCols = 64;
    static constexpr const char * kShort = "k_mmq6p", * kLong = "k_mmq6x";

    // an address's or a row offset's bytes past a dword, and an odd superblock's
    static __device__ __forceinline__ uint32_t mis(uint32_t a) { return a & 2; }
    static __device__ __forceinline__ int sb_odd(int sb) { return 2 * (sb & 1); }
    // the tile's staging dword i (dword dw of row `row`) in a stage buffer: the rows are packed
    static __device__ __forceinline__ int lds_slot(int i, int, int) { return i; }

    // block byte offset of a quarter's ql dwords (lb: + 32) and of its qh dwords, half 0
    static __device__ __forceinline__ constexpr int ql(int qi) { return L::QL + 64 * (qi >> 1) + 16 * (qi & 1); }
    static __device__ __forceinline__ constexpr int qh(int qi) { return L::QH + 32 * (qi >> 1) + 16 * (qi & 1); }

    // a lane's raw dwords of one superblock: per quarter the three aligned dwords covering its 8 bytes of
    // ql[..], ql[.. + 32] and qh[..]; the five covering the 16 scales and d
    struct Raw {
        uint32_t q[4][9];
        uint32_t s[5];
    };
    struct Head {
        uint32_t sc[4];  // the 16 scale bytes
    };
    // vo: the lane's row, at the block's dword
    static __device__ __forceinline__ void load_raw(Raw & o, __amdgpu_buffer_rsrc_t wres, uint32_t vo, int h, uint32_t so) {
#pragma unroll
        for (int qi = 0; qi < 4; qi++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                // (h is folded into the lane offset: the immediate part stays a constant)
                o.q[qi][i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + ql(qi) + 4 * i, so, 0);
                o.q[qi][3 + i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + ql(qi) + 32 + 4 * i, so, 0);
                o.q[qi][6 + i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + qh(qi) + 4 * i, so, 0);
            }
#pragma unroll
        for (int i = 0; i < 5; i++) o.s[i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + L::SC + 4 * i, so, 0);
    }
    // the raw dwords of the scales and d, and of quarter qi, from a lane's registers or from its row
    // in a stage buffer
    static __device__ __forceinline__ void raw_s(uint32_t (&s)[5], const Raw & o) {
#pragma unroll
        for (int i = 0; i < 5; i++) s[i] = o.s[i];
    }
    static __device__ __forceinline__ void raw_s(uint32_t (&s)[5], const uint32_t * blk) {
#pragma unroll
        for (int i = 0; i < 5; i++) s[i] = blk[L::SC / 4 + i];
    }
    static __device__ __forceinline__ void raw_q(uint32_t (&w)[9], const Raw & o, int qi, int) {
#pragma unroll
        for (int i = 0; i < 9; i++) w[i] = o.q[qi][i];
    }
    static __device__ __forceinline__ void raw_q(uint32_t (&w)[9], const uint32_t * blk, int qi, int h) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            w[i] = blk[ql(qi) / 4 + 2 * h + i];
            w[3 + i] = blk[ql(qi) / 4 + 8 + 2 * h + i];
            w[6 + i] = blk[qh(qi) / 4 + 2 * h + i];
        }
    }

    // the 16 scale bytes as four dwords, and d; off: the block's misalignment
    template <typename Src>
    static __device__ __forceinline__ float head(Head & hd, const Src & src, uint32_t off) {
        uint32_t s[5];
        raw_s(s, src);
#pragma unroll
        for (int i = 0; i < 4; i++) hd.sc[i] = __builtin_amdgcn_alignbyte(s[i + 1], s[i], off);
        return mi_h2f((uint16_t) ((s[4] >> (8 * off)) & 0xFFFF));
    }
    static __device__ __forceinline__ Op load_act(__amdgpu_buffer_rsrc_t xres, uint32_t vo, uint32_t so, int qi, int h) {
        return __builtin_bit_cast(long, __builtin_amdgcn_raw_buffer_load_b64(xres, vo + 16 * (qi & 1) + 8 * h, so, 0));
    }
    static __device__ __forceinline__ constexpr int act_blk(int qi, int t) { return 4 * (qi >> 1) + t; }
    static __device__ __forceinline__ i32x16 mfma(Op xa, Op b) { return __builtin_amdgcn_mfma_i32_32x32x16_i8(xa, b, i32x16{}, 0, 0, 0); }

    // T += sc_j D_j for the four sub-blocks of quarter qi: its operands op[t][0..1] = the lane's 8 bytes of
    // sub-block j as q - 32 from the nine raw dwords, then tile by tile
    template <int NT, typename Src>
    static __device__ __forceinline__ void phase(int (&T)[NT][16], Mins<NT> &, const Src & src, const Head & hd, const Op (&xa)[NT][4], int qi, int h, uint32_t off) {
        uint32_t w[9];
        raw_q(w, src, qi, h);
        int op[4][2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t la = __builtin_amdgcn_alignbyte(w[i + 1], w[i], off);
            const uint32_t lb = __builtin_amdgcn_alignbyte(w[3 + i + 1], w[3 + i], off);
            const uint32_t hh = __builtin_amdgcn_alignbyte(w[6 + i + 1], w[6 + i], off);
            qd_q6k_levels<2>(la, lb, hh, &op[0][i]);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ct++)
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int j = 8 * (qi >> 1) + 2 * t + (qi & 1);
                const long b = (long) (((unsigned long) (uint32_t) op[t][1] << 32) | (uint32_t) op[t][0]);
                sub_mad<sub_q6k>(T[ct], xa[ct][t], b, __builtin_amdgcn_sbfe(hd.sc[j >> 2], 8 * (j & 3), 8));
            }
    }
};

// IQ4_XS. Reference: ggml_vec_dot_iq4_xs_q8_K (src/ggml-quants.c:11873-11967): D_ib = sum_{e<32}
// kvalues[q[32 ib + e]] a[32 ib + e] with q the 4-bit codebook indices, kvalues the int8 levels
// kvalues_iq4nl (-127 .. 113) and s_ib = ls_ib - 32 from the 6-bit scales of the eight 32-element
// sub-blocks. A sub-block is exactly the K of v_mfma_i32_32x32x32_i8: |D_ib| <= 32 * 127 * 128 = 520 192 <
// 2^23, |T| <= 8 * 32 * 520 192 < 2^27: half the MFMAs and half the mads per superblock of Q6_K.
//
// Decode: the nibble layout is the lane halves'. Element j < 16 of sub-block ib is the low nibble of
// qs[16 ib + j], element 16 + j the high one: lane (r, h) takes the 16 qs bytes of its row's sub-block
// (four dwords: blocks are 136 bytes = 34 dwords of rows that start on a dword, so nothing is
// re-aligned), and mi_iq4nl_levels(w >> 4h) (three v_perm_b32 per four weights; it masks the other
// nibbles off itself) makes them its 16-byte operand, elements 16h .. 16h + 15, whose activations are
// the 16 bytes at 16h of 32-block ib, one b128 buffer load. No nibble is decoded twice. A phase is a
// half of the superblock, sub-blocks 4 hf + t; the scale and d_w come from the block's first two dwords
// (qd_iq4xs_scale). A staged row takes 36 dwords, the block from the third on, so its quants are
// 16-byte aligned.
struct sub_iq4xs : sub_no_mins {
    using Op = i32x4;
    static constexpr int BS = mi_type(MI_TYPE_IQ4_XS).bytes;  // 136
    static constexpr int kPhases = 2;
    static constexpr int kSlack = 0;
    static constexpr int kLoadDw = BS / 4;                       // dwords of a block
    static constexpr int kRowDw = kLoadDw + 2, kBlkDw = 2;       // a staged row: two of padding, then the block
    static_assert(BS % 4 == 0 && (kRowDw * 4) % 16 == 0, "IQ4_XS blocks are whole dwords; staged quants 16-byte aligned");
    // Prompts of up to 128 columns: k_mmqi4p; longer ones: k_mmqi4x, whose 256-column tiles cost the same
    // from 9 to 256 columns (profiles/iq4xs_prefill.txt, us per mul_mat, k_mmqi4p / k_mmqi4x: 4096 x 4096 B =
    // 64 9.4 / 15.6, B = 128 16.9 / 15.9, B = 512 62.3 / 32.1; 11008 x 4096 B = 64 18.4 / 37.6, B = 128 33.9 /
    // 38.1, B = 512 127.1 / 77.9: k_mmqi4p wins by 1.7-2x at 64, the shapes disagree at 128, k_mmqi4x wins
    // by 1.6-2x at 512).
    static constexpr int64_t kShortCols = 128;
    static constexpr const char * kShort = "k_mmqi4p", * kLong = "k_mmqi4x";

    static __device__ __forceinline__ uint32_t mis(uint32_t) { return 0; }
    static __device__ __forceinline__ int sb_odd(int) { return 0; }
    static __device__ __forceinline__ int lds_slot(int, int row, int dw) { return row * kRowDw + kBlkDw + dw; }

    // a lane's raw dwords of one superblock: the header (d | scales_h << 16, scales_l) and the 16 quant
    // bytes of each of the row's eight sub-blocks
    struct Raw {
        uint32_t hd, sl;
        uint4 q[8];
    };
    struct Head {
        uint32_t hd, sl;
    };
    static __device__ __forceinline__ void load_raw(Raw & o, __amdgpu_buffer_rsrc_t wres, uint32_t vo, int, uint32_t so) {
        o.hd = __builtin_amdgcn_raw_buffer_load_b32(wres, vo, so, 0);
        o.sl = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 4, so, 0);
#pragma unroll
        for (int ib = 0; ib < 8; ib++)
            o.q[ib] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wres, vo + 8 + 16 * ib, so, 0));
    }
    static __device__ __forceinline__ float head(Head & hd, const Raw & o, uint32_t) {
        hd.hd = o.hd;
        hd.sl = o.sl;
        return mi_h2f((uint16_t) (o.hd & 0xFFFF));
    }
    static __device__ __forceinline__ float head(Head & hd, const uint32_t * blk, uint32_t) {
        const uint2 v = *(const uint2 *) blk;
        hd.hd = v.x;
        hd.sl = v.y;
        return mi_h2f((uint16_t) (v.x & 0xFFFF));
    }
    // sub-block ib's 16 quant bytes from a lane's registers or from its row in a stage buffer
    static __device__ __forceinline__ uint4 raw_q(const Raw & o, int ib) { return o.q[ib]; }
    static __device__ __forceinline__ uint4 raw_q(const uint32_t * blk, int ib) { return *(const uint4 *) (blk + 2 + 4 * ib); }
    static __device__ __forceinline__ Op load_act(__amdgpu_buffer_rsrc_t xres, uint32_t vo, uint32_t so, int, int h) {
        return __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(xres, vo + 16 * h, so, 0));
    }
    static __device__ __forceinline__ constexpr int act_blk(int hf, int t) { return 4 * hf + t; }
    static __device__ __forceinline__ i32x16 mfma(Op xa, Op b) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(xa, b, i32x16{}, 0, 0, 0); }

    // T += (ls_ib - 32) D_ib for the four sub-blocks of half hf, each operand (the levels of the low, h =
    // 0, or the high nibbles) decoded once for every tile
    template <int NT, typename Src>
    static __device__ __forceinline__ void phase(int (&T)[NT][16], Mins<NT> &, const Src & src, const Head & hd, const Op (&xa)[NT][4], int hf, int h, uint32_t) {
        const int sh = 4 * h;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int ib = 4 * hf + t;
            const uint4 w = raw_q(src, ib);
            const i32x4 b = {mi_iq4nl_levels(w.x >> sh), mi_iq4nl_levels(w.y >> sh), mi_iq4nl_levels(w.z >> sh), mi_iq4nl_levels(w.w >> sh)};
            const int s = qd_iq4xs_scale(hd.sl, hd.hd >> 16, ib);
#pragma unroll
            for (int ct = 0; ct < NT; ct++) sub_mad<sub_iq4xs>(T[ct], xa[ct][t], b, s);
        }
    }
};

// Q3_K (sub_q3k) and Q2_K (sub_q2k). References: ggml_vec_dot_q3_K_q8_K (src/ggml-quants.c:6001-6103), D_j =
// sum_{e<16} (q - (hbit ? 0 : 4))[16j + e] a[16j + e] with levels in -4..3 and s_j = sc_j - 32 in -32..31:
// |D_j| <= 16 * 4 * 128 = 2^13, |T| <= 16 * 32 * 2^13 = 2^22; ggml_vec_dot_q2_K_q8_K (:5105-5169), levels q in
// 0..3, s_j = sc_j & 15, and the mins m_j = sc_j >> 4: |T| <= 16 * 15 * 16 * 3 * 128 < 2^21,
//     t = d_w T - dmin_w U,   U = sum_j m_j bsum_j,   bsum_j = sum_{e<16} a[16j + e]
// (mmqx_pre, the Q4_K family's form). v_mfma_i32_32x32x16_i8 as Q6_K.
//
// Decode (quant_decode.h: q23k_fmt, qd_q23k_levels): both pack the quants as Q6_K packs ql, so a phase is
// Q6_K's quarter (hq = qi / 2, u = qi % 2): the lane's 8 bytes of qs at 32 hq + 16u + 8h (Q3_K: and of hmask
// at 16u + 8h, the same for both hq) are the elements 8h .. 8h + 7 of the four sub-blocks j = 8 hq + 2t + u,
// whose activations are the 8 bytes at 16u + 8h of 32-block 4 hq + t: sub_q6k's load_act and act_blk.
// Q3_K blocks are 110 = 4 * 27 + 2 bytes, only 2-byte aligned, rows of an odd superblock count 2 mod 4:
// aligned dwords re-aligned with v_alignbyte as in sub_q6k, three covering a lane's 8 bytes, four the 12
// scale bytes and d. The 28 aligned dwords from a block's dword cover it at either misalignment (2 + 110 =
// 112 = 4 * 28); from an aligned block they end 2 bytes past it, inside the next block or the whole dword
// of slack that follows the tile's rows, as sub_q6k's. The scales are unpacked once per superblock
// into four dwords of int8 (qd_q3k_scales4), one v_bfe_i32 per sub-block. A staged row takes 29 dwords: an
// odd stride, as Q6_K's 53 and Q2_K's 21 are, so the 32 rows' same dword falls into 32 different banks.
// Q2_K blocks are 84 = 4 * 21 bytes of rows that are whole dwords (nb01 % 4 == 0): nothing is re-aligned,
// the scale is one v_bfe_u32 of the block's own dword.
//
// Q2_K's mins term is exact and needs no activation plane: lane (c, h) holds 8 of the 16 activation
// bytes of sub-block j of column c, so two v_dot4 against 0x02020202 are 2 P, P[j][h] their sum (|P| <=
// 1024) and bsum_j = P[j][0] + P[j][1]. P = 128 (P >> 7) + (P & 127) is two int8: byte 1 of 2 P and half
// of its byte 0, which v_perm_b32 gathers for the four sub-blocks of a phase into one dword each
// (Mins: hi[qi], lo[qi], byte t). After the phases two v_mfma_i32_32x32x32_i8 per tile, A = the sixteen
// P parts of the lane's column and half, B = the sixteen m_j of the lane's row in the same slots (qi, t)
// in both halves (Head::mn, qd_q2k_range4), give U = 128 U_hi + U_lo: the K slots sum over (j, h), so U
// comes out whatever K slot the hardware gives a byte. |U| <= 16 * 15 * 16 * 128 < 2^19: exact in f32.
template <int NT> struct q2k_mins {
    uint32_t hi[NT][4], lo[NT][4];
};
template <int TYPE>
struct sub_q23k : sub_no_mins {
    using L = q23k_fmt<TYPE>;
    static constexpr bool Q3 = L::Q3;
    using Op = long;
    static constexpr int BS = L::BS;
    static constexpr int kPhases = 4;
    static constexpr int kSlack = Q3 ? 4 : 0;                // Q3_K: the dword holding the last block's d
    static constexpr int kLoadDw = Q3 ? 28 : 21;             // aligned dwords of a block: 2 + 110 = 4 * 28; 84 = 4 * 21
    static constexpr int kRowDw = Q3 ? 29 : 21, kBlkDw = 0;  // a staged row: those dwords, an odd count of them
    static constexpr int NQ = Q3 ? 3 : 2;  // aligned dwords covering a lane's 8 bytes
    static constexpr int NS = Q3 ? 4 : 5;  // ... the 12 scale bytes and d; Q2_K: the 16 scale bytes, d | dmin
    static_assert(Q3 ? BS % 4 == 2 && 4 * kLoadDw == BS + 2 : 4 * kLoadDw == BS, "the aligned dwords of a block");
    // Prompts of up to 128 columns: the short shape; longer ones: the long shape (profiles/q2k_q3k_prefill.txt, us
    // per mul_mat, short / long. k_mmq3p / k_mmq3x: 4096 x 4096 B = 64 7.8 / 19.1, B = 128 13.1 / 19.5, B = 512 46.4 /
    // 38.0; 11008 x 4096 B = 64 19.9 / 52.4, B = 128 34.3 / 53.7, B = 512 118.9 / 98.2. k_mmq2p / k_mmq2x: 4096 x 4096
    // B = 64 10.3 / 20.5, B = 128 18.9 / 21.0, B = 512 70.0 / 41.1; 11008 x 4096 B = 64 21.3 / 52.2, B = 128 39.3 / 53.2,
    // B = 512 149.0 / 104.5: the short shape wins by 1.1-1.6x at 128, the long one by 1.2-1.7x at 512; nothing
    // between them was measured. The 8-column GEMV chunks every prompt of these types took before: 56-61 and
    // 149-150 at B = 64, 335-385 and 903-935 at B = 512.)
    static constexpr int64_t kShortCols = 128;
    static constexpr const char * kShort = Q3 ? "k_mmq3p" : "k_mmq2p", * kLong = Q3 ? "k_mmq3x" : "k_mmq2x";

    static __device__ __forceinline__ uint32_t mis(uint32_t a) { return Q3 ? a & 2 : 0; }
    static __device__ __forceinline__ int sb_odd(int sb) { return Q3 ? 2 * (sb & 1) : 0; }
    static __device__ __forceinline__ int lds_slot(int, int row, int dw) { return row * kRowDw + dw; }

    // block byte offset of a quarter's qs dwords and of a range's hmask dwords, half 0
    static __device__ __forceinline__ constexpr int qs(int qi) { return L::QS + 32 * (qi >> 1) + 16 * (qi & 1); }
    static __device__ __forceinline__ constexpr int hm(int u) { return 16 * u; }

    // a lane's raw dwords of one superblock: per quarter those covering its 8 bytes of qs, per range
    // those of hmask (Q3_K), and the scales' and d's
    struct Raw {
        uint32_t q[4][NQ];
        uint32_t hm[2][NQ];
        uint32_t s[NS];
    };
    struct Head {
        uint32_t sc[4];  // Q3_K: sc - 32 as int8, byte j; Q2_K: the scale bytes as they lie (sc | m << 4)
        uint32_t mn[4];  // Q2_K: the mins in slot order, byte t of dword qi
        float dm;        // Q2_K: dmin
    };
    // the phases' sums of the lane's activation bytes (Q2_K), split into two int8, slot order
    template <int NT> using Mins = std::conditional_t<Q3, sub_no_mins::Mins<NT>, q2k_mins<NT>>;
    static __device__ __forceinline__ void load_raw(Raw & o, __amdgpu_buffer_rsrc_t wres, uint32_t vo, int h, uint32_t so) {
#pragma unroll
        for (int i = 0; i < NQ; i++) {
#pragma unroll
            for (int qi = 0; qi < 4; qi++) o.q[qi][i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + qs(qi) + 4 * i, so, 0);
#pragma unroll
            for (int u = 0; u < 2; u++) o.hm[u][i] = Q3 ? __builtin_amdgcn_raw_buffer_load_b32(wres, vo + 8 * h + hm(u) + 4 * i, so, 0) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) o.s[i] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + L::SC + 4 * i, so, 0);
        if constexpr (!Q3) o.s[4] = __builtin_amdgcn_raw_buffer_load_b32(wres, vo + L::D, so, 0);
    }
    // the raw dwords of the scales and d, of quarter qi's quants and of its hmask range, from a lane's
    // registers or from its row in a stage buffer
    static __device__ __forceinline__ void raw_s(uint32_t (&s)[NS], const Raw & o) {
#pragma unroll
        for (int i = 0; i < NS; i++) s[i] = o.s[i];
    }
    static __device__ __forceinline__ void raw_s(uint32_t (&s)[NS], const uint32_t * blk) {
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = blk[L::SC / 4 + i];
        if constexpr (!Q3) s[4] = blk[L::D / 4];
    }
    static __device__ __forceinline__ void raw_q(uint32_t (&w)[2][NQ], const Raw & o, int qi, int) {
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            w[0][i] = o.q[qi][i];
            w[1][i] = o.hm[qi & 1][i];
        }
    }
    static __device__ __forceinline__ void raw_q(uint32_t (&w)[2][NQ], const uint32_t * blk, int qi, int h) {
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            w[0][i] = blk[qs(qi) / 4 + 2 * h + i];
            w[1][i] = Q3 ? blk[hm(qi & 1) / 4 + 2 * h + i] : 0u;
        }
    }

    // the scales (and Q2_K's mins and dmin) of a superblock, and d; off: the block's misalignment
    template <typename Src>
    static __device__ __forceinline__ float head(Head & hd, const Src & src, uint32_t off) {
        uint32_t s[NS];
        raw_s(s, src);
        if constexpr (Q3) {
            uint32_t a[3];
#pragma unroll
            for (int i = 0; i < 3; i++) a[i] = __builtin_amdgcn_alignbyte(s[i + 1], s[i], off);
#pragma unroll
            for (int g = 0; g < 4; g++) hd.sc[g] = qd_q3k_scales4(a[0], a[1], a[2], g);
            return mi_h2f((uint16_t) ((s[3] >> (8 * off)) & 0xFFFF));
        } else {
#pragma unroll
            for (int qi = 0; qi < 4; qi++) {
                hd.sc[qi] = s[qi];
                hd.mn[qi] = qd_nib_hi(qd_q2k_range4(s[2 * (qi >> 1)], s[2 * (qi >> 1) + 1], qi & 1));
            }
            hd.dm = mi_h2f((uint16_t) (s[4] >> 16));
            return mi_h2f((uint16_t) (s[4] & 0xFFFF));
        }
    }
    static __device__ __forceinline__ Op load_act(__amdgpu_buffer_rsrc_t xres, uint32_t vo, uint32_t so, int qi, int h) {
        return sub_q6k::load_act(xres, vo, so, qi, h);
    }
    static __device__ __forceinline__ constexpr int act_blk(int qi, int t) { return sub_q6k::act_blk(qi, t); }
    static __device__ __forceinline__ i32x16 mfma(Op xa, Op b) { return sub_q6k::mfma(xa, b); }

    // T += s_j D_j for the four sub-blocks of quarter qi: its operands op[t][0..1] = the lane's 8 bytes of
    // sub-block j as levels, then tile by tile; Q2_K: and the tile's P parts of the quarter
    template <int NT, typename Src>
    static __device__ __forceinline__ void phase(int (&T)[NT][16], Mins<NT> & ms, const Src & src, const Head & hd, const Op (&xa)[NT][4], int qi, int h, uint32_t off) {
        uint32_t w[2][NQ];
        raw_q(w, src, qi, h);
        int op[4][2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t q = Q3 ? __builtin_amdgcn_alignbyte(w[0][i + 1], w[0][i], off) : w[0][i];
            const uint32_t hb = Q3 ? __builtin_amdgcn_alignbyte(w[1][i + 1], w[1][i], off) : 0u;
#pragma unroll
            for (int t = 0; t < 4; t++) op[t][i] = qd_q23k_levels<Q3>(q, hb, qi >> 1, t);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ct++) {
            int p2[4];  // 2 P of the four sub-blocks
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int j = 8 * (qi >> 1) + 2 * t + (qi & 1);
                const long b = (long) (((unsigned long) (uint32_t) op[t][1] << 32) | (uint32_t) op[t][0]);
                const int s = Q3 ? __builtin_amdgcn_sbfe(hd.sc[j >> 2], 8 * (j & 3), 8) : (int) __builtin_amdgcn_ubfe(hd.sc[j >> 2], 8 * (j & 3), 4);
                sub_mad<sub_q23k>(T[ct], xa[ct][t], b, s);
                if constexpr (!Q3) p2[t] = mi_dot4(0x02020202, (int) xa[ct][t], mi_dot4(0x02020202, (int) (xa[ct][t] >> 32), 0));
            }
            if constexpr (!Q3) {
                // bytes 0 and 1 of p2[0..3]: [t0.b0 t1.b0 t0.b1 t1.b1] of each pair, then the b0s and the b1s
                const uint32_t p01 = __builtin_amdgcn_perm((uint32_t) p2[1], (uint32_t) p2[0], 0x05010400u);
                const uint32_t p23 = __builtin_amdgcn_perm((uint32_t) p2[3], (uint32_t) p2[2], 0x05010400u);
                ms.lo[ct][qi] = (__builtin_amdgcn_perm(p23, p01, 0x05040100u) >> 1) & 0x7F7F7F7Fu;
                ms.hi[ct][qi] = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
            }
        }
    }
    // U of tile ct (Q2_K): 128 U_hi + U_lo
    template <typename M>
    static __device__ __forceinline__ auto mins_term(const M & ms, const Head & hd, int ct) {
        if constexpr (Q3) {
            return NoU{};
        } else {
            const i32x4 b = {(int) hd.mn[0], (int) hd.mn[1], (int) hd.mn[2], (int) hd.mn[3]};
            const i32x4 ah = {(int) ms.hi[ct][0], (int) ms.hi[ct][1], (int) ms.hi[ct][2], (int) ms.hi[ct][3]};
            const i32x4 al = {(int) ms.lo[ct][0], (int) ms.lo[ct][1], (int) ms.lo[ct][2], (int) ms.lo[ct][3]};
            const i32x16 uh = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, b, i32x16{}, 0, 0, 0);
            const i32x16 ul = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, b, i32x16{}, 0, 0, 0);
            return uh * 128 + ul;
        }
    }
    using sub_no_mins::term;
    static __device__ __forceinline__ float term(int T, const i32x16 & U, int el, float dw, const Head & hd) {
        return mmqx_pre(T, (float) U[el], dw, hd.dm);
    }
};
using sub_q3k = sub_q23k<MI_TYPE_Q3_K>;
using sub_q2k = sub_q23k<MI_TYPE_Q2_K>;

template <typename F, int NT, bool STAGED>
__global__ __launch_bounds__(256, 2) void k_mmqs(mi_mmx_group grp) {
    MI_MMX_MEMBER(grp);
    using Op = typename F::Op;
    using Raw = typename F::Raw;
    constexpr int NW = 4;
    constexpr int NP = F::kPhases;
    static_assert(NP % 2 == 0, "the first phase of the next superblock goes into xa[0]");
    constexpr int TC = STAGED ? 32 * NT * NW : 32;  // columns per workgroup
    constexpr int kLoad = 32 * F::kLoadDw;          // dwords of a superblock of 32 rows
    constexpr int kStage = 32 * F::kRowDw;          // ... and of its stage buffer
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
    // results are not stored), so every load lies inside. Where blocks are not dword-aligned (F::mis),
    // the weights' base is the tile's first row aligned down to a dword; a block's dwords are then at
    // voff (lane: row offset, minus the block's misalignment) + soff (the superblock, a multiple of 4:
    // BS sb - F::sb_odd(sb), the other 2 bytes of an odd one in voff), and F::kSlack bytes follow the rows.
    const uint8_t * wt = W + n0 * nb01;
    const uint32_t bmis = F::mis((uint32_t) (uintptr_t) wt);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void *) (wt - bmis), (short) 0, (int) (bmis + nrows * nb01 + F::kSlack), 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xq, (short) 0, (int) (K * ncols), 0x00020000);
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc((void *) act.xd, (short) 0, (int) (S * ncols * 4), 0x00020000);
    auto row_off = [&](int row) { return bmis + (uint32_t) (std::min(row, nrows - 1) * nb01); };
    auto sb_soff = [](int sb) { return (uint32_t) __builtin_amdgcn_readfirstlane(sb * F::BS - F::sb_odd(sb)); };
    // this lane's row: its offset, its blocks' misalignment in an even superblock (an odd one: the other)
    const uint32_t wrow = row_off(r);
    const uint32_t rmis = F::mis(wrow);
    auto blk_mis = [&](int sb) { return rmis ^ (uint32_t) F::sb_odd(sb); };

    const uint32_t xstep = (uint32_t) ncols * 32;
    // the column's activation bytes of the four sub-blocks of phase p of superblock sb
    auto load_xa = [&](Op (&xa)[4], int sb, int p, uint32_t acol) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t so = (uint32_t) __builtin_amdgcn_readfirstlane((sb * 8 + F::act_blk(p, t)) * (int) xstep);
            xa[t] = F::load_act(xres, acol * 32, so, p, h);
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
    uint32_t acol[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ct++) acol[ct] = (uint32_t) std::min<int64_t>(c0 + 32 * ct + r, ncols - 1);
    Op xa[2][NT][4];
    // T of superblock sb from `src` (the lane's registers, or its row in a stage buffer); each phase's
    // activations are requested a phase ahead, the last one requests the first of superblock sn
    using Src = std::conditional_t<STAGED, const uint32_t *, Raw>;
    using Mins = typename F::template Mins<NT>;
    auto phases = [&](int (&T)[NT][16], Mins & ms, const Src & src, const typename F::Head & hd, int sb, int sn, uint32_t off) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
#pragma unroll
            for (int ct = 0; ct < NT; ct++) {
                if (p < NP - 1) load_xa(xa[(p + 1) & 1][ct], sb, p + 1, acol[ct]);
                else load_xa(xa[0][ct], sn, 0, acol[ct]);
            }
            F::template phase<NT>(T, ms, src, hd, xa[p & 1], p, h, off);
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
        auto load_raw = [&](Raw & o, int sb) { F::load_raw(o, wres, wrow - blk_mis(sb) + F::sb_odd(sb), h, sb_soff(sb)); };
        f32x16 gsum = {};
        if (nsb > 0) {
            Raw raw[2];
            load_raw(raw[0], sb_at(0));
            load_xa(xa[0][0], sb_at(0), 0, acol[0]);
            float dan = ld_d(sb_at(0), acol[0]);
            // the wave's k-th superblock from `cur`; superblock k + 1's raw dwords go into `nxt`
            auto step = [&](const Raw & cur, Raw & nxt, const int k) {
                const int sb = sb_at(k), sn = sb_at(k + 1);
                const bool first = sb % gs == 0, last = sb % gs == gs - 1 || sb == S - 1;
                load_raw(nxt, sn);
                const uint32_t off = blk_mis(sb);
                typename F::Head hd;
                const float dw = F::head(hd, cur, off);
                const float dac = dan;
                dan = ld_d(sn, acol[0]);
                int T[1][16] = {};
                Mins ms;
                phases(T, ms, cur, hd, sb, sn, off);
                const auto U = F::mins_term(ms, hd, 0);
                f32x16 da;
                spread_da(da, dac, dal[w][0]);
                if (first) {  // uniform: a group starts at -0 (-0 + t == t), kept a branch (no selects)
                    asm volatile("" ::: "memory");
                    gsum = f32x16(-0.0f);
                }
#pragma unroll
                for (int el = 0; el < 16; el++) gsum[el] = __builtin_fmaf(da[el], F::term(T[0][el], U, el, dw, hd), gsum[el]);
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
        // staging role: dword i = tid + 256 k of the superblock's 32 x kLoadDw = dword i % kLoadDw of row
        // i / kLoadDw, kept at F::lds_slot of a stage buffer
        float * parked = (float *) (lds + 2 * kStage) + w * NT * 16 * 64;
        uint32_t svo[kPasses];  // its byte offset in the tile's rows, of an even superblock
        int sls[kPasses];       // its dword in a stage buffer
        uint32_t sodd = 0;      // bit k: the row is misaligned (an odd superblock's dwords lie 4 bytes on)
#pragma unroll
        for (int k = 0; k < kPasses; k++) {
            const int i = std::min(tid + 256 * k, kLoad - 1);
            const int row = i / F::kLoadDw, dw = i - row * F::kLoadDw;
            const uint32_t ro = row_off(row);
            svo[k] = ro - F::mis(ro) + 4 * dw;
            sls[k] = F::lds_slot(tid + 256 * k, row, dw);
            sodd |= (F::mis(ro) >> 1) << k;
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
                if (tid + 256 * k < kLoad) lds[buf * kStage + sls[k]] = st[k];
        };

        f32x16 y[NT], gsum[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ct++) {
            y[ct] = f32x16(-0.0f);  // cfold_vec_park's first group sum lands exactly
            gsum[ct] = f32x16{};
        }
        uint32_t st[kPasses];
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
            const uint32_t * blk = lds + (sb & 1) * kStage + r * F::kRowDw + F::kBlkDw;
            const int sn = sb + 1 < S ? sb + 1 : S - 1;
            const uint32_t off = blk_mis(sb);
            typename F::Head hd;
            const float dw = F::head(hd, blk, off);
            int T[NT][16] = {};
            Mins ms;
            phases(T, ms, blk, hd, sb, sn, off);
            // the stage's successor into the other buffer (its readers passed the last barrier), then
            // the request for the one after
            store_stage(st, (sb + 1) & 1);
            load_stage(st, sb + 2);
#pragma unroll
            for (int ct = 0; ct < NT; ct++) {
                f32x16 da, tv;
                spread_da(da, dan[ct], dal[w][ct]);
                dan[ct] = ld_d(sn, acol[ct]);
                const auto U = F::mins_term(ms, hd, ct);
#pragma unroll
                for (int el = 0; el < 16; el++) tv[el] = F::term(T[ct][el], U, el, dw, hd);
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

// F's members (q8_K activations). Prompts of up to F::kShortCols columns, and every destination that
// is not local device memory: the short shape; longer ones: the long shape. kMmqShortKernels /
// kMmqLongKernels force either at any column count. Both follow the canonical combine order: the same
// bits.
template <typename F>
void mmqs_launch(mi_mmx_group & g, hipStream_t s, bool dst_local) {
    const int var = g_mi_tuning.mmq_variant;
    const int64_t ncols = g.m[0].act.ncols;
    if ((var & kMmqShortKernels) || (ncols <= F::kShortCols && !(var & kMmqLongKernels)) || !dst_local) {
        mi_route(F::kShort);
        hipLaunchKernelGGL((k_mmqs<F, 1, false>), dim3((unsigned) mmx_deal(g, 32, 32)), dim3(256), 0, s, g);
        return;
    }
    mi_route(F::kLong);
    hipLaunchKernelGGL((k_mmqs<F, 2, true>), dim3((unsigned) mmx_deal(g, 32, 256)), dim3(256), 0, s, g);
}

} // namespace

void mi_mmqs_group(mi_mmx_group & g, hipStream_t s, bool dst_local) {
    if (g.type == MI_TYPE_Q6_K) return mmqs_launch<sub_q6k>(g, s, dst_local);
    if (g.type == MI_TYPE_Q3_K) return mmqs_launch<sub_q3k>(g, s, dst_local);
    if (g.type == MI_TYPE_Q2_K) return mmqs_launch<sub_q2k>(g, s, dst_local);
    MI_ASSERT(g.type == MI_TYPE_IQ4_XS);
    mmqs_launch<sub_iq4xs>(g, s, dst_local);
}
