// mmv.hip -- GGML_OP_MUL_MAT for few activation columns (decode / GEMV regime) on gfx950.
//
// Memory-bound: every weight byte is read once from HBM, activations (a few KB per column)
// come from L1/L2. One wave64 owns one weight row; its lanes split the row into
// (superblock, 64-element group) items so that a K=4096 Q4_K row (16 superblocks x 4 groups)
// is exactly one item per lane, loaded with three aligned 16-byte loads per lane
// (header + 32 B of nibbles). Integer dot products use v_dot4_i32_i8 on the reference's own
// quantized activations, so each superblock's integer sum is bit-identical to
// ggml_vec_dot_q4_K_q8_K (src/ggml-quants.c:7007-7502); only the f32 combination order across
// superblocks differs from the CPU.
//
// Reference per-type dot products mirrored here:
//   Q4_0 x Q8_0  ggml_vec_dot_q4_0_q8_0  src/ggml-quants.c:3469-3874
//   Q8_0 x Q8_0  ggml_vec_dot_q8_0_q8_0  src/ggml-quants.c:4819+
//   Q4_1 x Q8_1  ggml_vec_dot_q4_1_q8_1  src/ggml-quants.c:4006-4039 (AVX2)
//   Q5_0 x Q8_0  ggml_vec_dot_q5_0_q8_0  src/ggml-quants.c:4279-4301 (AVX2)
//   Q5_1 x Q8_1  ggml_vec_dot_q5_1_q8_1  src/ggml-quants.c:4623-4648 (AVX2)
//   Q4_K x Q8_K  ggml_vec_dot_q4_K_q8_K  src/ggml-quants.c:7007-7502
//   Q5_K x Q8_K  ggml_vec_dot_q5_K_q8_K  src/ggml-quants.c:7833-8378
//   Q6_K x Q8_K  ggml_vec_dot_q6_K_q8_K  src/ggml-quants.c:8730-9310
//   Q2_K x Q8_K  ggml_vec_dot_q2_K_q8_K  src/ggml-quants.c:5105-5169
//   Q3_K x Q8_K  ggml_vec_dot_q3_K_q8_K  src/ggml-quants.c:6001-6103
//   IQ4_NL x Q8_0 ggml_vec_dot_iq4_nl_q8_0 src/ggml-quants.c:11733-11815
//   IQ4_XS x Q8_K ggml_vec_dot_iq4_xs_q8_K src/ggml-quants.c:11873-11967
// (F16 and F32 live in mmv_ordered.hip: bit-exact CPU summation order.)

#include <string>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

namespace {

constexpr int kRowsPerBlock = 4;  // 4 waves x 1 row
constexpr int kMaxCols = 8;

struct mmv_geom {
    int64_t K, N;
    int64_t ne11, ne12, ne13;
    int64_t r2, r3;          // broadcast ratios ne12/ne02, ne13/ne03
    size_t nb01, nb02, nb03;
    size_t nb1, nb2, nb3;
    int64_t col_chunks;      // ceil(ne11 / NC)
    mi_mm_ids id;            // MUL_MAT_ID (kernels instantiated with ID != 0)
};

// Decode blockIdx.y into (first column i11, i12, i13) and return the weight row pointer base.
__device__ __forceinline__ void mmv_coords(const mmv_geom & g, int NC, int64_t & i11, int64_t & i12, int64_t & i13,
                                           int64_t & i02, int64_t & i03) {
    const int64_t y = blockIdx.y;
    const int64_t chunk = y % g.col_chunks;
    const int64_t z = y / g.col_chunks;
    i12 = z % g.ne12;
    i13 = z / g.ne12;
    i11 = chunk * NC;
    i02 = i12 / g.r2;
    i03 = i13 / g.r3;
}

// What one workgroup's blockIdx.y stands for. ID 0: a chunk of NC consecutive columns of one
// (i12, i13) batch (mmv_coords). ID 1 (NC == 1): the MUL_MAT_ID pair (e, t) = (y % n_ids, y / n_ids).
// ID 2: a chunk of up to NC pairs of one expert, gathered by mi_mmid_group. A gathered column is
// only an index into the SoA activations and a destination address; each keeps its own accumulators.
template <int NC, int ID> struct mmv_item {
    int64_t i11, i12, i13;   // ID 0
    int64_t col0;            // ID 0: the first column's index in the activations
    int64_t wofs;            // byte offset of the weight matrix in W
    int n;                   // ID 2: pairs of this chunk
    int colx[ID ? NC : 1];   // ID 1 / 2: activation column per pair
    int pair[ID ? NC : 1];   // ID 1 / 2: the pair e + n_ids * t (32-bit and uniform: scalar registers)

    // false: nothing to do for this workgroup (an id outside [0, n_as), a chunk past the last one).
    // Uniform over the workgroup (blockIdx.y alone decides) and taken before any cross-lane operation.
    __device__ __forceinline__ bool init(const mmv_geom & g) {
        if constexpr (ID == 0) {
            int64_t i02, i03;
            mmv_coords(g, NC, i11, i12, i13, i02, i03);
            wofs = i02 * g.nb02 + i03 * g.nb03;
            col0 = i11 + g.ne11 * (i12 + g.ne12 * i13);
            return true;
        } else {
            int expert;
            const unsigned n_ids = (unsigned) g.id.n_ids, ne11 = (unsigned) g.ne11;
            if constexpr (ID == 1) {
                static_assert(NC == 1, "pairwise MUL_MAT_ID: one column per workgroup");
                n = 1;
                const unsigned e = blockIdx.y % n_ids, t = blockIdx.y / n_ids;
                expert = *(const int32_t *) ((const char *) g.id.ids + e * g.id.nb0 + t * g.id.nb1);
                pair[0] = (int) blockIdx.y;
                colx[0] = (int) (e % ne11 + ne11 * t);
            } else {
                const int4 ch = g.id.chunks[blockIdx.y];
                expert = ch.x;
                n = ch.z;
                if (n <= 0) return false;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const unsigned p = (unsigned) g.id.pairs[ch.y + (c < n ? c : 0)];
                    pair[c] = (int) p;
                    colx[c] = (int) ((p % n_ids) % ne11 + ne11 * (p / n_ids));
                }
            }
            if ((unsigned) expert >= (unsigned) g.id.n_as) return false;
            wofs = (int64_t) expert * g.nb02;
            return true;
        }
    }
    // column c of this workgroup exists (callers test it only for NC > 1)
    __device__ __forceinline__ bool has(const mmv_geom & g, int c) const {
        if constexpr (ID == 0) return i11 + c < g.ne11;
        else return c < n;
    }
    __device__ __forceinline__ int64_t col(int c) const {
        if constexpr (ID == 0) return col0 + c;
        else return colx[c];
    }
    __device__ __forceinline__ float * out(const mmv_geom & g, float * dst, int64_t row, int c) const {
        if constexpr (ID == 0) return (float *) ((char *) dst + (i11 + c) * g.nb1 + i12 * g.nb2 + i13 * g.nb3 + row * sizeof(float));
        else {
            const unsigned e = (unsigned) pair[c] % (unsigned) g.id.n_ids, t = (unsigned) pair[c] / (unsigned) g.id.n_ids;
            return (float *) ((char *) dst + e * g.nb1 + t * g.nb2 + row * sizeof(float));
        }
    }
};

template <int NC, int ID>
__device__ __forceinline__ void mmv_store(const mmv_geom & g, float * dst, int64_t row, const mmv_item<NC, ID> & it,
                                          float (&acc)[NC], int lane) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const float v = mi_wave_sum(acc[c]);
        if (lane == 0 && it.has(g, c)) *it.out(g, dst, row, c) = v;
    }
}

// ---------------------------------------------------------------- Q4_K / Q5_K x Q8_K

template <int NC, bool Q5, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_kq(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= g.N) return;
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    constexpr int BS = mi_type(Q5 ? MI_TYPE_Q5_K : MI_TYPE_Q4_K).bytes;
    const uint8_t * wrow = W + bi.wofs + row * g.nb01;
    const int nsb = (int) (g.K / 256);

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;

    for (int it = lane; it < 4 * nsb; it += 64) {
        const int s = it >> 2;
        const int j = it & 3;
        const uint8_t * blk = wrow + (size_t) s * BS;
        const uint4 hdr = *(const uint4 *) blk;
        const uint8_t * qp = blk + (Q5 ? 48 : 16) + 32 * j;
        const uint4 qa = *(const uint4 *) qp;
        const uint4 qb = *(const uint4 *) (qp + 16);
        uint32_t q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
        uint32_t qlo[8], qhi[8];
        if constexpr (Q5) {
            const uint4 ha = *(const uint4 *) (blk + 16);
            const uint4 hb = *(const uint4 *) (blk + 32);
            const uint32_t h[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
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
        const float dw = mi_h2f((uint16_t) (hdr.x & 0xFFFF));
        const float dmw = mi_h2f((uint16_t) (hdr.x >> 16));
        int sc0, m0, sc1, m1;
        mi_scale_min_k4(2 * j, hdr.y, hdr.z, hdr.w, sc0, m0);
        mi_scale_min_k4(2 * j + 1, hdr.y, hdr.z, hdr.w, sc1, m1);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int4 * a = (const int4 *) (act.qs + col * g.K + (int64_t) s * 256 + 64 * j);
            const int4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
            const int alo[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const int ahi[8] = {a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            int lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                lo = mi_dot4((int) qlo[i], alo[i], lo);
                hi = mi_dot4((int) qhi[i], ahi[i], hi);
            }
            const int sumi = sc0 * lo + sc1 * hi;
            const int ss = *(const int *) (act.s32 + col * (g.K / 32) + s * 8 + 2 * j);
            const int summ = m0 * (int) (int16_t) (ss & 0xFFFF) + m1 * (ss >> 16);
            const float dy = act.d[col * nsb + s];
            acc[c] += dy * (dw * (float) sumi - dmw * (float) summ);
        }
    }
    mmv_store<NC, ID>(g, dst, row, bi, acc, lane);
}

// ---------------------------------------------------------------- 32-element blocks x Q8_0 / Q8_1
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

// four fifth bits (bits 0..3 of x) to bit 4 of four bytes: bit b of x * 0x00204081 lands at b, b + 7,
// b + 14, b + 21 -- sixteen distinct positions, no carries -- of which 0, 8, 16, 24 are kept
__device__ __forceinline__ uint32_t q5_spread(uint32_t x) { return (((x & 0xFu) * 0x00204081u) & 0x01010101u) << 4; }

// 32 quants of a block starting at a 2-byte aligned address, gathered from aligned dwords.
template <int NBYTES>
__device__ __forceinline__ void load_qs_unaligned(const uint8_t * p, uint32_t (&out)[NBYTES / 4]) {
    const uintptr_t addr = (uintptr_t) p;
    const uint32_t * w = (const uint32_t *) (addr & ~(uintptr_t) 3);
    const int shift = (int) (addr & 3);  // 0 or 2 here
    uint32_t raw[NBYTES / 4 + 1];
#pragma unroll
    for (int i = 0; i < NBYTES / 4; i++) raw[i] = w[i];
    raw[NBYTES / 4] = shift ? w[NBYTES / 4] : 0u;  // buffers carry 256 B of tail slack
#pragma unroll
    for (int i = 0; i < NBYTES / 4; i++) out[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], shift);
}

template <int NC, int T, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q0(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    using F = q32_fmt<T>;
    constexpr bool Q8 = F::Q8;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= g.N) return;
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    constexpr int BS = F::BS;
    const uint8_t * wrow = W + bi.wofs + row * g.nb01;
    const int nb = (int) (g.K / 32);

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;

    for (int b = lane; b < nb; b += 64) {
        const uint8_t * blk = wrow + (size_t) b * BS;
        const float dw = mi_h2f(*(const uint16_t *) blk);
        int wq[8];
        if constexpr (Q8) {
            uint32_t t[8];
            load_qs_unaligned<32>(blk + 2, t);
#pragma unroll
            for (int i = 0; i < 8; i++) wq[i] = (int) t[i];
        } else {
            uint32_t t[4];
            load_qs_unaligned<16>(blk + F::QS, t);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if constexpr (F::LUT) {
                    mi_iq4nl_levels8(t[i], wq[i], wq[i + 4]);
                } else {
                    wq[i] = (int) (t[i] & 0x0F0F0F0Fu);          // elements 4i..4i+3
                    wq[i + 4] = (int) ((t[i] >> 4) & 0x0F0F0F0Fu);  // elements 16+4i..
                }
            }
            if constexpr (F::HAS_QH) {
                uint32_t qh[1];
                load_qs_unaligned<4>(blk + F::QH, qh);
#pragma unroll
                for (int i = 0; i < 8; i++) wq[i] |= (int) q5_spread(qh[0] >> (4 * i));
            }
        }
        float mw = 0.0f;
        if constexpr (F::HAS_M) mw = mi_h2f(*(const uint16_t *) (blk + 2));
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int4 * a = (const int4 *) (act.qs + col * g.K + (int64_t) b * 32);
            const int4 a0 = a[0], a1 = a[1];
            const int av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            int sumi = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) sumi = mi_dot4(wq[i], av[i], sumi);
            if constexpr (F::SUB != 0) {
                // (q - 8) * y summed = q*y - 8 * sum(y) (Q5_0: 16)
                int sy = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) sy = mi_dot4(0x01010101, av[i], sy);
                sumi -= F::SUB * sy;
            }
            acc[c] += (float) sumi * (dw * act.d[col * nb + b]);
            if constexpr (F::HAS_M) acc[c] += mw * mi_h2f((uint16_t) act.s32[col * nb + b]);  // m * s, the fp16-rounded s
        }
    }
    mmv_store<NC, ID>(g, dst, row, bi, acc, lane);
}

// Reference CPU order (mmv_order 1) for the Q4_0 / Q8_0 rows this generic path serves -- K % 256
// != 0 (rows of any block count, so only 2-byte aligned) and 3-D weight batches, where the fused
// reference-order kernel (mmv_fused_impl.h) does not apply. The reference's AVX2 dot
// (ggml_vec_dot_q8_0_q8_0 src/ggml-quants.c:4819+, ggml_vec_dot_q4_0_q8_0 :3469+) keeps eight
// float lanes: lane l gets the exact int32 sum of elements 4l..4l+3 of each block
// (mul_sum_i8_pairs_float; Q4_0 after bytes_from_nibbles_32 - 8: low nibbles of bytes 4l.. for
// l < 4, high nibbles of bytes 4(l-4).. for l >= 4) in acc[l] = fma(x.d * y.d, q, acc[l]) over the
// blocks in order, then hsum_float_8. Here eight lanes are those eight CPU lanes of one row (8 rows
// per wave): each runs its own chain, the hsum is three xor shuffles in the same pairing.
// Q5_0 (ggml_vec_dot_q5_0_q8_0 :4279-4301) is the same with the fifth bits or-ed in and 16 taken
// off. Q4_1 / Q5_1 (ggml_vec_dot_q4_1_q8_1 :4006-4039, _q5_1_q8_1 :4623-4648) keep the unsigned
// levels in the lanes and one scalar chain summs += fp16(x.m) * fp16(y.s) over the blocks in order
// (the product of two fp16 values is exact in f32, so a contracted fma gives the same bits); the
// result is hsum_float_8(acc) + summs.
// IQ4_NL (ggml_vec_dot_iq4_nl_q8_0 :11781-11815) looks the nibbles up in the codebook and keeps two
// accumulators: accum1 runs the chain over the even blocks, accum2 over the odd ones, and the result
// is hsum_float_8(accum1 + accum2). It walks the blocks in pairs, so the backend takes even block
// counts only.
template <int NC, int T, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q0_ord(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    using F = q32_fmt<T>;
    constexpr bool Q8 = F::Q8;
    const int l = threadIdx.x & 7;
    const int64_t row = (int64_t) blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = row < g.N;
    const int64_t rc = live ? row : g.N - 1;  // (dead groups run a valid row: no early exit before the shuffles)
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    constexpr int BS = F::BS;
    const uint8_t * wrow = W + bi.wofs + rc * g.nb01;
    const int nb = (int) (g.K / 32);
    // the lane's 4 quant bytes: block byte 2 + 4 l (nibble formats: QS + 4 (l & 3), nibble half l >> 2)
    const int qoff = F::QS + 4 * (Q8 ? l : (l & 3));

    float A[NC], M[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) A[c] = M[c] = 0.0f;

#pragma unroll 4
    for (int b = 0; b < nb; b++) {
        const uintptr_t blk = (uintptr_t) (wrow + (size_t) b * BS);
        // blocks are 2-byte aligned: d and the quants from the aligned dwords covering them
        // (buffers carry 256 B of tail slack)
        const uint32_t dw0 = *(const uint32_t *) (blk & ~(uintptr_t) 3);
        const float dw = mi_h2f((uint16_t) ((blk & 2) ? dw0 >> 16 : dw0 & 0xFFFF));
        const uintptr_t qa = blk + qoff;
        const uint32_t * qp = (const uint32_t *) (qa & ~(uintptr_t) 3);
        uint32_t q = __builtin_amdgcn_alignbyte(qp[1], qp[0], (uint32_t) (qa & 3));
        if constexpr (!Q8) q = (l < 4 ? q : q >> 4) & 0x0F0F0F0Fu;
        if constexpr (F::LUT) q = (uint32_t) mi_iq4nl_levels(q);
        float mw = 0.0f;
        if constexpr (F::HAS_M) mw = mi_h2f((uint16_t) ((blk & 2) ? *(const uint32_t *) (blk + 2) & 0xFFFF : dw0 >> 16));
        if constexpr (F::HAS_QH) {
            const uintptr_t ha = blk + F::QH;
            const uint32_t * hp = (const uint32_t *) (ha & ~(uintptr_t) 3);
            const uint32_t qh = (ha & 3) ? __builtin_amdgcn_alignbyte(hp[1], hp[0], (uint32_t) (ha & 3)) : hp[0];
            q |= q5_spread(qh >> (4 * l));  // elements 4l..4l+3: bits 4l.. of qh
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int av = *(const int *) (act.qs + col * g.K + (int64_t) b * 32 + 4 * l);
            // Q4_0: (q - 8) . y, exact (0xF8 = -8 per byte); Q5_0: (q - 16) . y (0xF0)
            constexpr int kSub = (int) (F::SUB == 16 ? 0xF0F0F0F0u : 0xF8F8F8F8u);
            const int sumi = F::SUB == 0 ? mi_dot4((int) q, av, 0) : mi_dot4((int) q, av, mi_dot4(kSub, av, 0));
            if (F::LUT && (b & 1)) M[c] = fmaf(dw * act.d[col * nb + b], (float) sumi, M[c]);  // accum2: the odd blocks
            else A[c] = fmaf(dw * act.d[col * nb + b], (float) sumi, A[c]);  // _mm256_fmadd_ps, exact int -> float
            if constexpr (F::HAS_M) M[c] = M[c] + mw * mi_h2f((uint16_t) act.s32[col * nb + b]);  // summs += x.m * y.s (exact product)
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        const float a = F::LUT ? A[c] + M[c] : A[c];  // IQ4_NL: _mm256_add_ps(accum1, accum2)
        float z = a + __shfl_xor(a, 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        if constexpr (F::HAS_M) z = z + M[c];
        if (l == 0 && live && bi.has(g, c)) *bi.out(g, dst, row, c) = z;
    }
}

// Reference-order Q4_K / Q5_K mul_mat for the shapes the fused stream kernel does not take (3-D
// weight batches broadcast over r2 / r3, strided src1): the reference's AVX2 vec_dot
// (ggml-quants.c:7089-7152 Q4_K, :7920-8002 Q5_K) keeps eight int32 lanes `sumi` per superblock,
// lane l = sum over the four 64-element chunks j of sc[2j] * (4 low-nibble products at 4l..4l+3) +
// sc[2j+1] * (4 high-nibble products), then acc[l] = fma(d, (float) sumi[l], acc[l]) with
// d = y.d * fp16(x.d); the mins go to four f32 lanes acc_m[k] = fma(dmin, (float) (m[2k] S[2k] +
// m[2k+1] S[2k+1]), acc_m[k]) (Q4_K; dmin = -y.d * fp16(x.dmin)), or to one scalar the -mfma build
// contracts, summs = fma(dmin, (float) sum_k prod[k], summs) (Q5_K). Result hsum_float_8(acc) +
// ((acc_m0 + acc_m2) + (acc_m1 + acc_m3)), resp. + summs. Here eight lanes are the eight CPU lanes
// of one row (8 rows per wave), lanes 0..3 also the four acc_m lanes.
template <int NC, bool Q5, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_kq_ord(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    const int l = threadIdx.x & 7;
    const int64_t row = (int64_t) blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = row < g.N;
    const int64_t rc = live ? row : g.N - 1;  // (dead groups run a valid row: no early exit before the shuffles)
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    constexpr int BS = mi_type(Q5 ? MI_TYPE_Q5_K : MI_TYPE_Q4_K).bytes;
    const uint8_t * wrow = W + bi.wofs + rc * g.nb01;
    const int nsb = (int) (g.K / 256);

    float A[NC], M[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) A[c] = M[c] = 0.0f;

    for (int s = 0; s < nsb; s++) {
        const uint8_t * blk = wrow + (size_t) s * BS;
        const uint4 hdr = *(const uint4 *) blk;
        const float dw = mi_h2f((uint16_t) (hdr.x & 0xFFFF));
        const float dmw = mi_h2f((uint16_t) (hdr.x >> 16));
        uint32_t qlo[4], qhi[4];
        int sc[8], mn[8];
#pragma unroll
        for (int j = 0; j < 8; j++) mi_scale_min_k4(j, hdr.y, hdr.z, hdr.w, sc[j], mn[j]);
        const uint32_t hb = Q5 ? *(const uint32_t *) (blk + 16 + 4 * l) : 0u;  // qh bytes 4l..4l+3
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = *(const uint32_t *) (blk + (Q5 ? 48 : 16) + 32 * j + 4 * l);
            qlo[j] = q & 0x0F0F0F0Fu;
            qhi[j] = (q >> 4) & 0x0F0F0F0Fu;
            if constexpr (Q5) {
                qlo[j] |= ((hb >> (2 * j)) & 0x01010101u) << 4;
                qhi[j] |= ((hb >> (2 * j + 1)) & 0x01010101u) << 4;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int8_t * aq = act.qs + col * g.K + (int64_t) s * 256 + 4 * l;
            int sumi = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int lo = mi_dot4((int) qlo[j], *(const int *) (aq + 64 * j), 0);
                const int hi = mi_dot4((int) qhi[j], *(const int *) (aq + 64 * j + 32), 0);
                sumi += sc[2 * j] * lo + sc[2 * j + 1] * hi;  // madd(scale_l, p16l) + madd(scale_h, p16h)
            }
            const float ya = act.d[col * nsb + s];
            A[c] = fmaf(ya * dw, (float) sumi, A[c]);  // _mm256_fmadd_ps(d, cvt(sumi), acc)
            const float dmin = -ya * dmw;
            const int16_t * S = act.s32 + col * (g.K / 32) + (int64_t) s * 8;
            if constexpr (!Q5) {
                if (l < 4) {
                    const int prod = mn[2 * l] * (int) S[2 * l] + mn[2 * l + 1] * (int) S[2 * l + 1];
                    M[c] = fmaf(dmin, (float) prod, M[c]);  // _mm_fmadd_ps(dmin, cvt(prod), acc_m)
                }
            } else {
                int tot = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) tot += mn[j] * (int) S[j];
                M[c] = fmaf(dmin, (float) tot, M[c]);  // summs += dmin * hsum(prod), contracted
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A[c] + __shfl_xor(A[c], 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        float m = M[c];
        if constexpr (!Q5) {
            // acc_m + movehl(acc_m), then lane 0 + lane 1: (m0 + m2) + (m1 + m3)
            m = m + __shfl_xor(m, 2, 8);
            m = m + __shfl_xor(m, 1, 8);
        }
        if (l == 0 && live && bi.has(g, c)) *bi.out(g, dst, row, c) = z + m;
    }
}

// ---------------------------------------------------------------- Q6_K x Q8_K
//
// ggml_vec_dot_q6_K_q8_K (src/ggml-quants.c:8838-8915, the AVX2 branch). A 210-byte block is
// ql[128] | qh[64] | int8 scales[16] | fp16 d; element e of the superblock is
// d * scales[e / 16] * (q - 32) with q in 0..63. For the 128-half h, byte p (0..31):
//   ql[64h + p]      low nibble -> element 128h + p,      high nibble -> element 128h + 64 + p
//   ql[64h + 32 + p] low nibble -> element 128h + 32 + p, high nibble -> element 128h + 96 + p
//   qh[32h + p]      bits 2t, 2t+1 -> bits 4, 5 of element 128h + 32t + p
// Blocks are only 2-byte aligned (210 = 2 * 105; rows of an odd superblock count are 2 mod 4):
// every load is an aligned dword (+ v_alignbyte) or narrower, never a uint4 on a block address.

// bytes of q (each 0..63) -> bytes of q - 32 as int8, no carries between the bytes:
// (q + 128 - 32) never borrows, the xor takes the 128 back out mod 256
__device__ __forceinline__ int q6_center(uint32_t q) { return (int) (((q | 0x80808080u) - 0x20202020u) ^ 0x80808080u); }

// a dword at a 2-byte aligned address from the two aligned dwords covering it
__device__ __forceinline__ uint32_t ld32_a2(const uint8_t * p) {
    const uintptr_t a = (uintptr_t) p;
    const uint32_t * w = (const uint32_t *) (a & ~(uintptr_t) 3);
    const uint32_t lo = w[0];
    const uint32_t hi = (a & 3) ? w[1] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t) (a & 3));
}

// Tree order: one wave per row, an item is (superblock s, 128-half h, 16-byte lane range u): the
// four 16-element sub-blocks at elements 128h + 32t + 16u (t = 0..3), scale index 8h + 2t + u.
// Four items per superblock, so a K = 4096 row is one item per lane. The item's integer sum
// (up to 4 * 8,323,072, over 2^24) is accumulated in int32 and converted once.
template <int NC, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q6k(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= g.N) return;
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + row * g.nb01;
    const int nsb = (int) (g.K / 256);

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;

    for (int it = lane; it < 4 * nsb; it += 64) {
        const int s = it >> 2;
        const int h = (it >> 1) & 1;
        const int u = it & 1;
        const uint8_t * blk = wrow + (size_t) s * mi_type(MI_TYPE_Q6_K).bytes;
        uint32_t la[4], lb[4], hh[4];
        load_qs_unaligned<16>(blk + 64 * h + 16 * u, la);
        load_qs_unaligned<16>(blk + 64 * h + 32 + 16 * u, lb);
        load_qs_unaligned<16>(blk + 128 + 32 * h + 16 * u, hh);
        int q[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            q[0][i] = q6_center((la[i] & 0x0F0F0F0Fu) | ((hh[i] & 0x03030303u) << 4));
            q[1][i] = q6_center((lb[i] & 0x0F0F0F0Fu) | (((hh[i] >> 2) & 0x03030303u) << 4));
            q[2][i] = q6_center(((la[i] >> 4) & 0x0F0F0F0Fu) | (((hh[i] >> 4) & 0x03030303u) << 4));
            q[3][i] = q6_center(((lb[i] >> 4) & 0x0F0F0F0Fu) | (((hh[i] >> 6) & 0x03030303u) << 4));
        }
        const int8_t * scp = (const int8_t *) blk + 192 + 8 * h + u;
        const int sc[4] = {scp[0], scp[2], scp[4], scp[6]};
        const float dw = mi_h2f(*(const uint16_t *) (blk + 208));
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int4 * a = (const int4 *) (act.qs + col * g.K + (int64_t) s * 256 + 128 * h + 16 * u);
            int sumi = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int4 av = a[2 * t];
                int p = mi_dot4(q[t][0], av.x, 0);
                p = mi_dot4(q[t][1], av.y, p);
                p = mi_dot4(q[t][2], av.z, p);
                p = mi_dot4(q[t][3], av.w, p);
                sumi += sc[t] * p;
            }
            acc[c] += (act.d[col * nsb + s] * dw) * (float) sumi;
        }
    }
    mmv_store<NC, ID>(g, dst, row, bi, acc, lane);
}

// Reference order: the AVX2 dot keeps eight int32 lanes per superblock, lane l = sum over the
// eight 32-element groups g of scales[2g + (l >= 4)] * sum_{e = 4l..4l+3} (q - 32)[32g + e] * a[32g + e]
// (maddubs pairs, the -32 taken as maddubs(32, a) and subtracted, then madd_epi16 with the
// sign-extended scales: no step saturates, |pair| <= 2 * 63 * 127), then acc[l] = fma(y.d * fp16(x.d),
// (float) sumi[l], acc[l]) over the superblocks in order and hsum_float_8. A lane sum is at most
// 8 * 128 * 4 * 32 * 127 = 16,646,144 < 2^24, so the conversion is exact. Here eight lanes are the
// eight CPU lanes of one row (8 rows per wave), as k_mmv_kq_ord.
template <int NC, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q6k_ord(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    const int l = threadIdx.x & 7;
    const int64_t row = (int64_t) blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = row < g.N;
    const int64_t rc = live ? row : g.N - 1;  // (dead groups run a valid row: no early exit before the shuffles)
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + rc * g.nb01;
    const int nsb = (int) (g.K / 256);
    const int hi = l >> 2;  // which 16-element half of each 32-group the lane's elements lie in

    float A[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) A[c] = 0.0f;

    for (int s = 0; s < nsb; s++) {
        const uint8_t * blk = wrow + (size_t) s * mi_type(MI_TYPE_Q6_K).bytes;
        const float dw = mi_h2f(*(const uint16_t *) (blk + 208));
        int q[8], sc[8];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t la = ld32_a2(blk + 64 * h + 4 * l);
            const uint32_t lb = ld32_a2(blk + 64 * h + 32 + 4 * l);
            const uint32_t hh = ld32_a2(blk + 128 + 32 * h + 4 * l);
            q[4 * h + 0] = q6_center((la & 0x0F0F0F0Fu) | ((hh & 0x03030303u) << 4));
            q[4 * h + 1] = q6_center((lb & 0x0F0F0F0Fu) | (((hh >> 2) & 0x03030303u) << 4));
            q[4 * h + 2] = q6_center(((la >> 4) & 0x0F0F0F0Fu) | (((hh >> 4) & 0x03030303u) << 4));
            q[4 * h + 3] = q6_center(((lb >> 4) & 0x0F0F0F0Fu) | (((hh >> 6) & 0x03030303u) << 4));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) sc[j] = ((const int8_t *) blk)[192 + 2 * j + hi];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int8_t * aq = act.qs + col * g.K + (int64_t) s * 256 + 4 * l;
            int sumi = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) sumi += sc[j] * mi_dot4(q[j], *(const int *) (aq + 32 * j), 0);
            A[c] = fmaf(act.d[col * nsb + s] * dw, (float) sumi, A[c]);  // _mm256_fmadd_ps(d, cvt(sumi), acc)
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A[c] + __shfl_xor(A[c], 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        if (l == 0 && live && bi.has(g, c)) *bi.out(g, dst, row, c) = z;
    }
}

// ---------------------------------------------------------------- Q2_K / Q3_K x Q8_K
//
// ggml_vec_dot_q2_K_q8_K (src/ggml-quants.c:5105-5169) and ggml_vec_dot_q3_K_q8_K (:6001-6103), the
// AVX2 branches. Q2_K (84 B): scales[16] | qs[64] | fp16 d | fp16 dmin, element d (sc & 0xF) q -
// dmin (sc >> 4) with q in 0..3. Q3_K (110 B): hmask[32] | qs[64] | scales[12] | fp16 d, element
// d (sc - 32) (q - (hbit ? 0 : 4)) with the 6-bit sc as q3k_scale unpacks it. Both pack the quants
// alike: byte qs[32h + b] holds at bit 2t element 128h + 32t + b (h = 0..1, t = 0..3, b = 0..31);
// bit 4h + t of hmask[b] is that element's high bit. Q2_K blocks are 4-byte aligned, Q3_K blocks
// 2-byte aligned (rows of an odd superblock count are 2 mod 4): aligned dwords (+ v_alignbyte) or
// narrower loads only, as Q6_K.
template <int T> struct q23k_fmt {
    static constexpr bool Q3 = T == MI_TYPE_Q3_K;
    static constexpr int BS = mi_type(T).bytes;
    static constexpr int QS = Q3 ? 32 : 16;   // offset of qs
    static constexpr int SC = Q3 ? 96 : 0;    // offset of scales
    static constexpr int D = Q3 ? 108 : 80;   // offset of d (Q2_K: dmin follows)
};

// sub-block t's quants of a dword of qs (and, Q3_K, of the hmask dword of the same bytes, high bit
// 4h + t) as int8x4: Q2_K q in 0..3; Q3_K (q | hbit << 2) - 4 = q - (hbit ? 0 : 4), no carries
// between the bytes ((v + 128 - 4) never borrows, the xor takes the 128 back out)
template <bool Q3>
__device__ __forceinline__ int q23k_quants(uint32_t qs, uint32_t hm, int h, int t) {
    const uint32_t q = (qs >> (2 * t)) & 0x03030303u;
    if constexpr (!Q3) return (int) q;
    else return (int) (((q | (((hm >> (4 * h + t)) & 0x01010101u) << 2) | 0x80808080u) - 0x04040404u) ^ 0x80808080u);
}

// Q3_K: sub-block j's scale minus 32 -- low four bits in the nibbles of scales[0..7], upper two in
// scales[8 + j % 4] at bit 2 (j / 4) (the kmask1 / kmask2 unpack of the reference)
__device__ __forceinline__ int q3k_scale(const uint8_t * scales, int j) {
    const int lo = (scales[j & 7] >> (4 * (j >> 3))) & 0xF;
    return (lo | (((scales[8 + (j & 3)] >> (2 * (j >> 2))) & 3) << 4)) - 32;
}

// Tree order: Q6_K's item (superblock s, 128-half h, 16-byte range u), item = 4s + 2h + u. It
// reads qs[32h + 16u ..+15] (and hmask[16u ..+15]): the four 16-element sub-blocks at elements
// 128h + 32t + 16u, scales index 8h + 2t + u. All integer sums are exact in f32 (an item is at most
// 4 * 16 * 4 * 128 * 32 = 2^20). Q2_K's mins term needs the 16-element sums of the activations,
// which act.s32 (sums of 32) does not hold: v_dot4 of the quants in hand against 0x01010101.
template <int NC, int T, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q23k(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    using F = q23k_fmt<T>;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= g.N) return;
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + row * g.nb01;
    const int nsb = (int) (g.K / 256);

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;

    for (int it = lane; it < 4 * nsb; it += 64) {
        const int s = it >> 2;
        const int h = (it >> 1) & 1;
        const int u = it & 1;
        const uint8_t * blk = wrow + (size_t) s * F::BS;
        uint32_t qs[4], hm[4] = {0u, 0u, 0u, 0u};
        load_qs_unaligned<16>(blk + F::QS + 32 * h + 16 * u, qs);
        if constexpr (F::Q3) load_qs_unaligned<16>(blk + 16 * u, hm);
        int q[4][4], sc[4], mn[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int i = 0; i < 4; i++) q[t][i] = q23k_quants<F::Q3>(qs[i], hm[i], h, t);
            if constexpr (F::Q3) {
                sc[t] = q3k_scale(blk + F::SC, 8 * h + 2 * t + u);
                mn[t] = 0;
            } else {
                const int b = blk[8 * h + 2 * t + u];
                sc[t] = b & 0xF;
                mn[t] = b >> 4;
            }
        }
        const float dw = mi_h2f(*(const uint16_t *) (blk + F::D));
        const float dmw = F::Q3 ? 0.0f : mi_h2f(*(const uint16_t *) (blk + F::D + 2));
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int4 * a = (const int4 *) (act.qs + col * g.K + (int64_t) s * 256 + 128 * h + 16 * u);
            int sumi = 0, summ = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int4 av = a[2 * t];
                int p = mi_dot4(q[t][0], av.x, 0);
                p = mi_dot4(q[t][1], av.y, p);
                p = mi_dot4(q[t][2], av.z, p);
                p = mi_dot4(q[t][3], av.w, p);
                sumi += sc[t] * p;
                if constexpr (!F::Q3) {
                    int b16 = mi_dot4(0x01010101, av.x, 0);
                    b16 = mi_dot4(0x01010101, av.y, b16);
                    b16 = mi_dot4(0x01010101, av.z, b16);
                    b16 = mi_dot4(0x01010101, av.w, b16);
                    summ += mn[t] * b16;
                }
            }
            acc[c] += act.d[col * nsb + s] * (dw * (float) sumi - dmw * (float) summ);
        }
    }
    mmv_store<NC, ID>(g, dst, row, bi, acc, lane);
}

// Reference order: both AVX2 dots keep eight int32 lanes per superblock, lane l = sum over the
// eight 32-element groups g of S[2g + (l >= 4)] * sum_{e = 4l..4l+3} Q[32g + e] * a[32g + e], with
// (S, Q) = (sc & 0xF, q) for Q2_K and (sc - 32, q - 4 * !hbit) for Q3_K (maddubs pairs -- Q3_K's
// high-bit part as a second maddubs, subtracted -- then madd_epi16 with the scales: no step
// saturates), then acc[l] = fma(y.d * fp16(x.d), (float) sumi[l], acc[l]) over the superblocks and
// hsum_float_8. Q2_K first adds its mins on the same accumulator: acc[l] = fma(-y.d * fp16(x.dmin),
// (float) (m[2l] * bsums[2l] + m[2l+1] * bsums[2l+1]), acc[l]), m the high nibbles of scales and
// bsums the 16-element sums of the Q8_K block (here: of the quants, which is what they are).
// A lane sum is at most 8 * 4 * 4 * 128 * 32 = 2^19 and a mins product below 2^16: exact in f32.
// Eight lanes are the eight CPU lanes of one row (8 rows per wave), as k_mmv_q6k_ord.
template <int NC, int T, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_q23k_ord(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    using F = q23k_fmt<T>;
    const int l = threadIdx.x & 7;
    const int64_t row = (int64_t) blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = row < g.N;
    const int64_t rc = live ? row : g.N - 1;  // (dead groups run a valid row: no early exit before the shuffles)
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + rc * g.nb01;
    const int nsb = (int) (g.K / 256);
    const int hi = l >> 2;  // which 16-element half of each 32-group the lane's elements lie in

    float A[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) A[c] = 0.0f;

    for (int s = 0; s < nsb; s++) {
        const uint8_t * blk = wrow + (size_t) s * F::BS;
        const float dw = mi_h2f(*(const uint16_t *) (blk + F::D));
        const float dmw = F::Q3 ? 0.0f : mi_h2f(*(const uint16_t *) (blk + F::D + 2));
        const uint32_t hm = F::Q3 ? ld32_a2(blk + 4 * l) : 0u;
        int q[8], sc[8];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t qs = ld32_a2(blk + F::QS + 32 * h + 4 * l);
#pragma unroll
            for (int t = 0; t < 4; t++) q[4 * h + t] = q23k_quants<F::Q3>(qs, hm, h, t);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) sc[j] = F::Q3 ? q3k_scale(blk + F::SC, 2 * j + hi) : (blk[2 * j + hi] & 0xF);
        int m0 = 0, m1 = 0;
        if constexpr (!F::Q3) {
            m0 = blk[2 * l] >> 4;
            m1 = blk[2 * l + 1] >> 4;
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int8_t * aq = act.qs + col * g.K + (int64_t) s * 256;
            const float ya = act.d[col * nsb + s];
            if constexpr (!F::Q3) {
                const int4 b0 = *(const int4 *) (aq + 32 * l), b1 = *(const int4 *) (aq + 32 * l + 16);
                const int s0 = mi_dot4(0x01010101, b0.w, mi_dot4(0x01010101, b0.z, mi_dot4(0x01010101, b0.y, mi_dot4(0x01010101, b0.x, 0))));
                const int s1 = mi_dot4(0x01010101, b1.w, mi_dot4(0x01010101, b1.z, mi_dot4(0x01010101, b1.y, mi_dot4(0x01010101, b1.x, 0))));
                A[c] = fmaf(-ya * dmw, (float) (m0 * s0 + m1 * s1), A[c]);  // _mm256_fmadd_ps(dmin, cvt(prod), acc)
            }
            int sumi = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) sumi += sc[j] * mi_dot4(q[j], *(const int *) (aq + 32 * j + 4 * l), 0);
            A[c] = fmaf(ya * dw, (float) sumi, A[c]);  // _mm256_fmadd_ps(d, cvt(sumi), acc)
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A[c] + __shfl_xor(A[c], 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        if (l == 0 && live && bi.has(g, c)) *bi.out(g, dst, row, c) = z;
    }
}

// ---------------------------------------------------------------- IQ4_XS x Q8_K
//
// ggml_vec_dot_iq4_xs_q8_K (src/ggml-quants.c:11873-11967). IQ4_XS (136 B): fp16 d | u16 scales_h |
// scales_l[4] | qs[128]; sub-block ib (32 elements, quants qs[16 ib ..], element j < 16 the low
// nibble of byte j, element 16 + j its high nibble) has the 6-bit scale ls = (nibble ib of scales_l)
// | (bits 2 ib .. of scales_h) << 4 and the value d (ls - 32) kvalues_iq4nl[q]. Blocks are whole
// dwords (136 = 4 * 34) of rows that start on one.
__device__ __forceinline__ int iq4xs_scale(uint32_t sl, uint32_t sh, int ib) {
    return (int) (((sl >> (4 * ib)) & 0xF) | (((sh >> (2 * ib)) & 3) << 4)) - 32;
}

// Tree order: item (superblock s, quarter u) = 4 s + u: the sub-blocks 2u and 2u + 1, 32 bytes of
// quants, looked up once and used for every column. A sub-block's sum is below 32 * 127 * 127 * 32 <
// 2^24: exact in f32.
template <int NC, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_iq4xs(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    constexpr int BS = mi_type(MI_TYPE_IQ4_XS).bytes;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= g.N) return;
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + row * g.nb01;
    const int nsb = (int) (g.K / 256);

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;

    for (int it = lane; it < 4 * nsb; it += 64) {
        const int s = it >> 2, u = it & 3;
        const uint32_t * blk = (const uint32_t *) (wrow + (size_t) s * BS);
        const uint32_t h0 = blk[0], sl = blk[1];
        const float dw = mi_h2f((uint16_t) (h0 & 0xFFFF));
        const int ls0 = iq4xs_scale(sl, h0 >> 16, 2 * u), ls1 = iq4xs_scale(sl, h0 >> 16, 2 * u + 1);
        int lv[16];  // [0..7] sub-block 2u (elements 4i.. in lv[i]), [8..15] sub-block 2u + 1
#pragma unroll
        for (int i = 0; i < 4; i++) {
            mi_iq4nl_levels8(blk[2 + 8 * u + i], lv[i], lv[4 + i]);
            mi_iq4nl_levels8(blk[6 + 8 * u + i], lv[8 + i], lv[12 + i]);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int4 * a = (const int4 *) (act.qs + col * g.K + (int64_t) s * 256 + 64 * u);
            const int4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
            const int av[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
            int p0 = 0, p1 = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                p0 = mi_dot4(lv[i], av[i], p0);
                p1 = mi_dot4(lv[8 + i], av[8 + i], p1);
            }
            acc[c] += (dw * act.d[col * nsb + s]) * ((float) (ls0 * p0) + (float) (ls1 * p1));
        }
    }
    mmv_store<NC, ID>(g, dst, row, bi, acc, lane);
}

// Reference order, the AVX2 branch: per superblock eight int32 lanes, lane l = sum over the eight
// sub-blocks ib of (ls_ib - 32) * sum_{e = 4l..4l+3} v[32 ib + e] a[32 ib + e] (mul_add_epi8 pairs,
// at most 2 * 127 * 127: no saturation; madd_epi16 with the scale) -- for l < 4 the low nibbles of
// bytes 4l.. of the sub-block, for l >= 4 the high nibbles of bytes 4(l - 4).. -- then
// acc[l] = fma(fp16(x.d) * y.d, (float) sumi[l], acc[l]) over the superblocks and hsum_float_8. A lane
// sum is below 8 * 4 * 127 * 127 * 32 < 2^24: exact in f32. Eight lanes are the eight CPU lanes of
// one row (8 rows per wave), as k_mmv_q6k_ord.
template <int NC, int ID = 0>
__global__ __launch_bounds__(256) void k_mmv_iq4xs_ord(const uint8_t * __restrict__ W, mi_act_q8 act, float * __restrict__ dst, mmv_geom g) {
    constexpr int BS = mi_type(MI_TYPE_IQ4_XS).bytes;
    const int l = threadIdx.x & 7;
    const int64_t row = (int64_t) blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = row < g.N;
    const int64_t rc = live ? row : g.N - 1;  // (dead groups run a valid row: no early exit before the shuffles)
    mmv_item<NC, ID> bi;
    if (!bi.init(g)) return;
    const uint8_t * wrow = W + bi.wofs + rc * g.nb01;
    const int nsb = (int) (g.K / 256);

    float A[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) A[c] = 0.0f;

    for (int s = 0; s < nsb; s++) {
        const uint32_t * blk = (const uint32_t *) (wrow + (size_t) s * BS);
        const uint32_t h0 = blk[0], sl = blk[1];
        const float dw = mi_h2f((uint16_t) (h0 & 0xFFFF));
        int lv[8], sc[8];
#pragma unroll
        for (int ib = 0; ib < 8; ib++) {
            const uint32_t q = blk[2 + 4 * ib + (l & 3)];
            lv[ib] = mi_iq4nl_levels((l < 4 ? q : q >> 4) & 0x0F0F0F0Fu);
            sc[ib] = iq4xs_scale(sl, h0 >> 16, ib);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (NC > 1 && !bi.has(g, c)) break;
            const int64_t col = bi.col(c);
            const int8_t * aq = act.qs + col * g.K + (int64_t) s * 256;
            int sumi = 0;
#pragma unroll
            for (int ib = 0; ib < 8; ib++) sumi += sc[ib] * mi_dot4(lv[ib], *(const int *) (aq + 32 * ib + 4 * l), 0);
            A[c] = fmaf(dw * act.d[col * nsb + s], (float) sumi, A[c]);  // _mm256_fmadd_ps(d, cvt(sumi), accum)
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
        float z = A[c] + __shfl_xor(A[c], 4, 8);
        z = z + __shfl_xor(z, 2, 8);
        z = z + __shfl_xor(z, 1, 8);
        if (l == 0 && live && bi.has(g, c)) *bi.out(g, dst, row, c) = z;
    }
}

mmv_geom make_geom(const mi_mm_desc & m, int NC) {
    mmv_geom g;
    g.K = m.K;
    g.N = m.N;
    g.ne11 = m.ne11;
    g.ne12 = m.ne12;
    g.ne13 = m.ne13;
    g.r2 = m.ne12 / m.ne02;
    g.r3 = m.ne13 / m.ne03;
    g.nb01 = m.nb01;
    g.nb02 = m.nb02;
    g.nb03 = m.nb03;
    g.nb1 = m.nb1;
    g.nb2 = m.nb2;
    g.nb3 = m.nb3;
    g.col_chunks = (m.ne11 + NC - 1) / NC;
    g.id = m.id;
    return g;
}

} // namespace

// One launch of weight type T's GEMV (its family by the table: 32-element blocks, Q6_K, Q2_K / Q3_K, IQ4_XS, Q4_K / Q5_K) in
// tree order (a wave per row) or the reference CPU's order (ORD: 8 rows per wave), NC columns per
// workgroup. ID as mmv_item; grid_y 0: the column chunks of every (i12, i13) batch.
template <int T, int NC, int ID, bool ORD>
static void mmv_launch(const mi_mm_desc & m, const mi_act_q8 & act, unsigned grid_y, hipStream_t s) {
    const mmv_geom g = make_geom(m, NC);
    const dim3 grid((unsigned) (ORD ? (m.N + 31) / 32 : (m.N + kRowsPerBlock - 1) / kRowsPerBlock),
                    grid_y ? grid_y : (unsigned) (g.col_chunks * m.ne12 * m.ne13));
    const uint8_t * W = (const uint8_t *) m.W;
    constexpr bool Q5 = T == MI_TYPE_Q5_K;
    // the route's name, built once per instance: kernel family, order, columns per workgroup, MUL_MAT_ID form
    static const std::string route = std::string(mi_type(T).blck == 32 ? "k_mmv_q0" : T == MI_TYPE_Q6_K ? "k_mmv_q6k" :
                                                 T == MI_TYPE_Q2_K || T == MI_TYPE_Q3_K ? "k_mmv_q23k" : T == MI_TYPE_IQ4_XS ? "k_mmv_iq4xs" : "k_mmv_kq") +
                                     (ORD ? "_ord" : "") + "<nc" + std::to_string(NC) + (ID == 1 ? ",id_pairs" : ID == 2 ? ",id_grouped" : "") + ">";
    mi_route(route.c_str());
    if constexpr (mi_type(T).blck == 32) {
        if constexpr (ORD) hipLaunchKernelGGL((k_mmv_q0_ord<NC, T, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
        else hipLaunchKernelGGL((k_mmv_q0<NC, T, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
    } else if constexpr (T == MI_TYPE_Q6_K) {
        if constexpr (ORD) hipLaunchKernelGGL((k_mmv_q6k_ord<NC, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
        else hipLaunchKernelGGL((k_mmv_q6k<NC, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
    } else if constexpr (T == MI_TYPE_Q2_K || T == MI_TYPE_Q3_K) {
        if constexpr (ORD) hipLaunchKernelGGL((k_mmv_q23k_ord<NC, T, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
        else hipLaunchKernelGGL((k_mmv_q23k<NC, T, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
    } else if constexpr (T == MI_TYPE_IQ4_XS) {
        if constexpr (ORD) hipLaunchKernelGGL((k_mmv_iq4xs_ord<NC, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
        else hipLaunchKernelGGL((k_mmv_iq4xs<NC, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
    } else {
        if constexpr (ORD) hipLaunchKernelGGL((k_mmv_kq_ord<NC, Q5, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
        else hipLaunchKernelGGL((k_mmv_kq<NC, Q5, ID>), grid, dim3(256), 0, s, W, act, m.dst, g);
    }
}

// GGML_OP_MUL_MAT_ID: pair by pair (ID 1, one column per workgroup), or, with the device-built
// chunk table, up to chunk_cap (8 or 4) gathered columns of one expert per workgroup (ID 2; the grid covers the
// worst-case chunk count, workgroups past the real one exit at once). Same per-column arithmetic as
// the plain kernels in both orders.
template <int T, bool ORD>
static void mmv_launch_ids(const mi_mm_desc & m, const mi_act_q8 & act, hipStream_t s) {
    const int64_t pairs = (int64_t) m.id.n_ids * m.ne12;
    if (!m.id.chunks) mmv_launch<T, 1, 1, ORD>(m, act, (unsigned) pairs, s);
    else if (m.id.chunk_cap == 4) mmv_launch<T, 4, 2, ORD>(m, act, (unsigned) mi_mmid_max_chunks(m.id.n_as, pairs, 4), s);
    else mmv_launch<T, 8, 2, ORD>(m, act, (unsigned) mi_mmid_max_chunks(m.id.n_as, pairs, m.id.chunk_cap), s);
}

// A plain mul_mat: columns per workgroup by the column count. Tree order 1, 2, 3, 4 or 8; the
// reference order 1, 2, 4 or 8.
template <int T, bool ORD>
static void mmv_launch_cols(const mi_mm_desc & m, const mi_act_q8 & act, hipStream_t s) {
    switch (m.ne11 >= 5 ? 8 : (int) m.ne11) {
        case 1: mmv_launch<T, 1, 0, ORD>(m, act, 0, s); break;
        case 2: mmv_launch<T, 2, 0, ORD>(m, act, 0, s); break;
        case 3: mmv_launch<T, ORD ? 4 : 3, 0, ORD>(m, act, 0, s); break;
        case 4: mmv_launch<T, 4, 0, ORD>(m, act, 0, s); break;
        default: mmv_launch<T, 8, 0, ORD>(m, act, 0, s); break;
    }
}

// The counting sort of the reference's MUL_MAT_ID (src/ggml.c:12169-12184: per-expert row lists in
// (t, e) order) as one workgroup. The ids are staged through LDS in tiles; thread x scans them for
// the experts x, x + 256, ... (every thread reads the same LDS word: a broadcast), first counting,
// then, after the exclusive sums over the experts, writing its experts' pair lists in the
// reference's order and their chunks of at most `cap` pairs. Chunk entries past the last real one get
// count 0. Ids outside [0, n_as) are in no list.
constexpr int kMmidTile = 4096;
__global__ __launch_bounds__(256) void k_mmid_group(mi_mm_ids id, int n_tokens, int max_chunks, int cap, int4 * __restrict__ chunks,
                                                    int32_t * __restrict__ pairs) {
    __shared__ int tile[kMmidTile];
    __shared__ int cnt[kMiMmidMaxExperts];
    __shared__ int first[kMiMmidMaxExperts];   // start of the expert's pair list
    __shared__ int chunk0[kMiMmidMaxExperts];  // its first chunk
    __shared__ int nchunks;
    const int tid = threadIdx.x;
    const int P = id.n_ids * n_tokens;
    for (int x = tid; x < id.n_as; x += 256) cnt[x] = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (int base = 0; base < P; base += kMmidTile) {
            const int nt = P - base < kMmidTile ? P - base : kMmidTile;
            __syncthreads();
            for (int i = tid; i < nt; i += 256) {
                const int p = base + i;
                const int64_t e = p % id.n_ids, t = p / id.n_ids;
                tile[i] = *(const int32_t *) ((const char *) id.ids + e * id.nb0 + t * id.nb1);
            }
            __syncthreads();
            for (int x = tid; x < id.n_as; x += 256) {
                int c = cnt[x];
                if (pass == 0) {
                    for (int i = 0; i < nt; i++) c += tile[i] == x;
                } else {
                    for (int i = 0; i < nt; i++) {
                        if (tile[i] == x) pairs[c++] = base + i;
                    }
                }
                cnt[x] = c;
            }
        }
        __syncthreads();
        if (pass == 0) {
            if (tid == 0) {
                int f = 0, ch = 0;
                for (int x = 0; x < id.n_as; x++) {
                    first[x] = f;
                    chunk0[x] = ch;
                    f += cnt[x];
                    ch += (cnt[x] + cap - 1) / cap;
                }
                nchunks = ch;
            }
            __syncthreads();
            for (int x = tid; x < id.n_as; x += 256) {
                const int n = cnt[x];
                for (int k = 0; cap * k < n; k++) chunks[chunk0[x] + k] = make_int4(x, first[x] + cap * k, n - cap * k < cap ? n - cap * k : cap, 0);
                cnt[x] = first[x];  // pass 1: the write cursor
            }
            for (int k = nchunks + tid; k < max_chunks; k += 256) chunks[k] = make_int4(0, 0, 0, 0);
        }
    }
}

void mi_mmid_group(const mi_mm_ids & id, int64_t n_tokens, int4 * chunks, int32_t * pairs, hipStream_t s) {
    hipLaunchKernelGGL(k_mmid_group, dim3(1), dim3(256), 0, s, id, (int) n_tokens,
                       (int) mi_mmid_max_chunks(id.n_as, (int64_t) id.n_ids * n_tokens, id.chunk_cap), id.chunk_cap, chunks, pairs);
}

void mi_mul_mat_q(const mi_mm_desc & m, const mi_act_q8 & act, hipStream_t s) {
    const bool ord = mi_mmv_order() == 1;
    mi_dispatch_type(m.type, [&](auto t) {
        constexpr int T = decltype(t)::value;
        if constexpr (mi_type_quantized(T)) {
            if (m.id.ids && ord) mmv_launch_ids<T, true>(m, act, s);
            else if (m.id.ids) mmv_launch_ids<T, false>(m, act, s);
            else if (ord) mmv_launch_cols<T, true>(m, act, s);
            else mmv_launch_cols<T, false>(m, act, s);
        } else {
            MI_ASSERT(!"mi_mul_mat_q: not a quantized weight type");
        }
    });
}
