// mm_bf16.hip -- BF16 weights x bf16 activations (GGML_TYPE_BF16, vec_dot_type BF16).
//
// The reference rounds an F32 src1 to bf16 rows (ggml_fp32_to_bf16_row, src/ggml-impl.h:75-92) and
// dots them with ggml_vec_dot_bf16 (src/ggml.c:1610-1672). A product of two bf16 values has 16
// significant bits: it is exact in f32 unless it underflows, so the orders below differ only in how
// the f32 sums are arranged.
//
//   k_convert_bf16   src1 columns (F32 / F16 / BF16, any strides mi_src_cols describes) -> bf16 rows
//                    [ncols][K] with ggml_fp32_to_bf16's bits (integer arithmetic: NaNs made quiet,
//                    a zero exponent field flushed to a signed zero, else round to nearest even);
//                    BF16 columns are copied as they lie
//   k_mm_bf16_ord    mmv_order 1, any shape: ggml_vec_dot_bf16 as the reference's AVX2 build runs it
//                    (read off the built object): 4 registers x 8 lanes of vfmadd231ps over steps of 32,
//                    (c1 + c3) + (c2 + c4), upper + lower half, g + movehl(g), lane 0 + lane 1, to
//                    double, then the K % 32 leftovers as doubles of separately rounded f32 products
//                    (vmulss, vcvtss2sd, vaddsd), cast to float. A quad of lanes plays the 4 registers.
//                    Also the generic kernel of the tree order: weight batches, MUL_MAT_ID, rows that
//                    are not 16-byte aligned, K % 8 != 0.
//   k_gemv_bf16      tree order, 1..8 columns, 2-D: 16 lanes per weight row, 4 rows per wave, 16-byte
//                    weight loads of a whole tile requested before the first arithmetic, activations
//                    staged once per workgroup in LDS, bits << 16 and v_fma_f32
//   k_mm_bf16p       tree order, more than 8 columns, 2-D: 32 x 32 tiles on v_mfma_f32_32x32x16_bf16,
//                    the 64-deep K chunks dealt round-robin to the tile's 4 waves, partial tiles added
//                    in wave order

#include <algorithm>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#include "cpu_order.h"

namespace {

using namespace mi_cpu;

typedef float float16v __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // (a HIP uint4 array is not promoted to registers)

// ---------------------------------------------------------------------------------------------
// activation converter
// ---------------------------------------------------------------------------------------------

template <int SRC>  // MI_TYPE_F32, MI_TYPE_F16 or MI_TYPE_BF16
__global__ __launch_bounds__(256) void k_convert_bf16(mi_src_cols x, int64_t K, uint16_t * __restrict__ out) {
    const int64_t col = blockIdx.x;
    const int64_t i1 = col % x.ne1, i2 = (col / x.ne1) % x.ne2, i3 = col / (x.ne1 * x.ne2);
    const char * src = x.base + i1 * x.nb1 + i2 * x.nb2 + i3 * x.nb3;
    for (int64_t k = (int64_t) blockIdx.y * 256 + threadIdx.x; k < K; k += (int64_t) gridDim.y * 256) {
        uint16_t b;
        if constexpr (SRC == MI_TYPE_BF16) b = ((const uint16_t *) src)[k];
        else if constexpr (SRC == MI_TYPE_F16) b = mi_f2bf(mi_h2f(((const uint16_t *) src)[k]));
        else b = mi_f2bf(((const float *) src)[k]);
        out[col * K + k] = b;
    }
}

// ---------------------------------------------------------------------------------------------
// reference order (and the generic kernel)
// ---------------------------------------------------------------------------------------------

constexpr int kQuadsPerBlock = 64;  // 256 threads

struct bf_geom {
    int64_t K, N;
    int64_t ne11, ne12, ne13;
    int64_t r2, r3;
    size_t nb01, nb02, nb03;
    size_t nb1, nb2, nb3;
    int64_t col_chunks;
    mi_mm_ids id;
};

template <class V>  // uint4 or u32x4
__device__ __forceinline__ void b8_to_f(const V & b, float (&f)[8]) {
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void ld_b8(const uint16_t * p, float (&f)[8]) {
    if constexpr (ALIGNED) {
        b8_to_f(*(const uint4 *) p, f);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) f[i] = mi_bf2f(p[i]);
    }
}

// the AVX2 tail of ggml_vec_dot_bf16 over a quad's 4 x 8 lane sums (lane q holds register c_{q+1})
__device__ __forceinline__ float quad_reduce_bf16(float (&v)[8]) {
#pragma unroll
    for (int l = 0; l < 8; l++) v[l] = add_rn(v[l], __shfl_xor(v[l], 2, 64));  // c1 + c3, c2 + c4
#pragma unroll
    for (int l = 0; l < 8; l++) v[l] = add_rn(v[l], __shfl_xor(v[l], 1, 64));  // (c1 + c3) + (c2 + c4)
    const float g0 = add_rn(v[4], v[0]), g1 = add_rn(v[5], v[1]), g2 = add_rn(v[6], v[2]), g3 = add_rn(v[7], v[3]);
    return add_rn(add_rn(g0, g2), add_rn(g1, g3));  // g + movehl(g, g), then lane 0 + lane 1
}

// One quad per (row, chunk of NC columns); xb: [ncols][K] bf16 rows. blockIdx.y: the column chunk and the
// batch (i12, i13), or, IDS, the pair (e, t) of a MUL_MAT_ID (an id outside [0, n_as) skips the pair).
template <int NC, bool ALIGNED, bool IDS>
__global__ __launch_bounds__(256) void k_mm_bf16_ord(const uint8_t * __restrict__ W, const uint16_t * __restrict__ xb,
                                                     float * __restrict__ dst, bf_geom g) {
    const int q = threadIdx.x & 3;
    const int64_t row = (int64_t) blockIdx.x * kQuadsPerBlock + (threadIdx.x >> 2);
    const bool live = row < g.N;
    int64_t i11, i12, i13, wofs, col0;
    int nc;
    if constexpr (IDS) {
        static_assert(NC == 1, "MUL_MAT_ID: one column per workgroup");
        i11 = blockIdx.y % g.id.n_ids;
        i12 = blockIdx.y / g.id.n_ids;
        const int expert = *(const int32_t *) ((const char *) g.id.ids + i11 * g.id.nb0 + i12 * g.id.nb1);
        if ((unsigned) expert >= (unsigned) g.id.n_as) return;  // blockIdx.y alone decides: the whole workgroup leaves
        wofs = (int64_t) expert * (int64_t) g.nb02;
        i13 = 0;
        col0 = i11 % g.ne11 + g.ne11 * i12;
        nc = 1;
    } else {
        const int64_t y = blockIdx.y;
        const int64_t chunk = y % g.col_chunks;
        const int64_t z = y / g.col_chunks;
        i12 = z % g.ne12, i13 = z / g.ne12;
        i11 = chunk * NC;
        wofs = (i12 / g.r2) * g.nb02 + (i13 / g.r3) * g.nb03;
        col0 = i11 + g.ne11 * (i12 + g.ne12 * i13);
        nc = (int) (g.ne11 - i11);
        nc = nc > NC ? NC : nc;
    }
    const uint16_t * wrow = (const uint16_t *) (W + wofs + (live ? row : 0) * g.nb01);

    float acc[NC][8];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int l = 0; l < 8; l++) acc[c][l] = 0.0f;

    const int64_t np = g.K & ~(int64_t) 31;
    for (int64_t i = 8 * q; i < np; i += 32) {
        float w[8];
        ld_b8<ALIGNED>(wrow + i, w);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c < nc) {
                float x[8];
                ld_b8<ALIGNED>(xb + (col0 + c) * g.K + i, x);
#pragma unroll
                for (int l = 0; l < 8; l++) acc[c][l] = __fmaf_rn(w[l], x[l], acc[c][l]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const float r = quad_reduce_bf16(acc[c]);
        if (q == 0 && live && c < nc) {
            double s = (double) r;
            for (int64_t i = np; i < g.K; i++) s += (double) mul_rn(mi_bf2f(wrow[i]), mi_bf2f(xb[(col0 + c) * g.K + i]));
            *(float *) ((char *) dst + (i11 + c) * g.nb1 + i12 * g.nb2 + i13 * g.nb3 + row * sizeof(float)) = (float) s;
        }
    }
}

bf_geom make_geom(const mi_mm_desc & m, int NC) {
    bf_geom g;
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

bool rows_aligned(const mi_mm_desc & m, const uint16_t * xb) {
    return m.K >= 8 && m.K % 8 == 0 && ((uintptr_t) m.W | m.nb01 | m.nb02 | m.nb03 | (uintptr_t) xb) % 16 == 0;
}

template <int NC> void launch_ord(const mi_mm_desc & m, const uint16_t * xb, hipStream_t s) {
    const bf_geom g = make_geom(m, NC);
    const int64_t ny = g.col_chunks * m.ne12 * m.ne13;
    MI_ASSERT(ny <= 65535 && "BF16 mul_mat: too many column chunks for one launch");
    const dim3 grid((unsigned) ((m.N + kQuadsPerBlock - 1) / kQuadsPerBlock), (unsigned) ny);
    if (rows_aligned(m, xb)) hipLaunchKernelGGL((k_mm_bf16_ord<NC, true, false>), grid, dim3(256), 0, s, (const uint8_t *) m.W, xb, m.dst, g);
    else hipLaunchKernelGGL((k_mm_bf16_ord<NC, false, false>), grid, dim3(256), 0, s, (const uint8_t *) m.W, xb, m.dst, g);
}

void mul_mat_ord(const mi_mm_desc & m, const uint16_t * xb, hipStream_t s) {
    if (m.id.ids) {  // MUL_MAT_ID: pair by pair
        const bf_geom g = make_geom(m, 1);
        const dim3 grid((unsigned) ((m.N + kQuadsPerBlock - 1) / kQuadsPerBlock), (unsigned) ((int64_t) m.id.n_ids * m.ne12));
        if (rows_aligned(m, xb)) hipLaunchKernelGGL((k_mm_bf16_ord<1, true, true>), grid, dim3(256), 0, s, (const uint8_t *) m.W, xb, m.dst, g);
        else hipLaunchKernelGGL((k_mm_bf16_ord<1, false, true>), grid, dim3(256), 0, s, (const uint8_t *) m.W, xb, m.dst, g);
        return;
    }
    switch (m.ne11 >= 4 ? 4 : (int) m.ne11) {
        case 1: launch_ord<1>(m, xb, s); break;
        case 2: launch_ord<2>(m, xb, s); break;
        case 3: launch_ord<3>(m, xb, s); break;
        default: launch_ord<4>(m, xb, s); break;
    }
}

// ---------------------------------------------------------------------------------------------
// decode GEMV, tree order
// ---------------------------------------------------------------------------------------------

// A workgroup of 4 waves serves 16 rows: 16 lanes per row, lane p the 16-byte chunks p + 16 j of the row.
// A tile is U chunks per lane (U x 128 elements of K): its U loads are issued together (every load
// unconditional, at a clamped address; a chunk past the row is zeroed by a select) before the tile's
// arithmetic. The NC activation columns are copied into LDS once per workgroup as bf16.
template <int NC, int U>
__global__ __launch_bounds__(256) void k_gemv_bf16(const uint8_t * __restrict__ W, size_t nb01, int64_t K, int64_t N,
                                                   const uint16_t * __restrict__ xb, float * __restrict__ dst, size_t ycol) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    u32x4 * xs = (u32x4 *) smem;  // [NC][K / 8]
    const int nch = (int) (K / 8);  // 16-byte chunks per row
    for (int i = threadIdx.x; i < NC * nch; i += 256) xs[i] = ((const u32x4 *) xb)[i];
    const int p = threadIdx.x & 15;
    const int64_t row = (int64_t) blockIdx.x * 16 + (threadIdx.x >> 4);
    const u32x4 * wrow = (const u32x4 *) (W + std::min<int64_t>(row, N - 1) * nb01);
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0f;
    __syncthreads();
    for (int j0 = 0; j0 < nch; j0 += 16 * U) {
        u32x4 wv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int j = j0 + 16 * u + p;
            wv[u] = wrow[j < nch ? j : nch - 1];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int j = j0 + 16 * u + p;
            const bool in = j < nch;
            if (!in) wv[u] = (u32x4) (0u);
            float w[8];
            b8_to_f(wv[u], w);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float x[8];
                b8_to_f(xs[c * nch + (in ? j : 0)], x);
#pragma unroll
                for (int l = 0; l < 8; l++) acc[c] = __fmaf_rn(w[l], x[l], acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float v = acc[c];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (p == 0 && row < N) *(float *) ((char *) dst + c * ycol + row * sizeof(float)) = v;
    }
}

constexpr size_t kGemvLds = 48 * 1024;  // the staged columns: 2 K bytes each

template <int NC> void launch_gemv(const mi_mm_desc & m, const uint16_t * xb, float * dst, hipStream_t s) {
    const dim3 grid((unsigned) ((m.N + 15) / 16));
    const size_t lds = (size_t) NC * m.K * 2;
    if (m.K <= 1024) hipLaunchKernelGGL((k_gemv_bf16<NC, 4>), grid, dim3(256), lds, s, (const uint8_t *) m.W, m.nb01, m.K, m.N, xb, dst, m.nb1);
    else hipLaunchKernelGGL((k_gemv_bf16<NC, 8>), grid, dim3(256), lds, s, (const uint8_t *) m.W, m.nb01, m.K, m.N, xb, dst, m.nb1);
}

bool gemv_supported(const mi_mm_desc & m, const uint16_t * xb) {
    return !m.id.ids && m.ne02 == 1 && m.ne03 == 1 && m.ne12 == 1 && m.ne13 == 1 && m.ne11 <= 8 && rows_aligned(m, xb) &&
           (size_t) m.K * 2 <= kGemvLds && m.N >= 1 && (m.N + 15) / 16 <= INT32_MAX;
}

void mul_mat_gemv(const mi_mm_desc & m, const uint16_t * xb, hipStream_t s) {
    // as many columns per launch as the LDS budget stages (8 at K <= 3072, 1 from K > 12288 on)
    const int cap = (int) std::min<size_t>(8, kGemvLds / ((size_t) m.K * 2));
    for (int64_t c0 = 0; c0 < m.ne11; c0 += cap) {
        const int nc = (int) std::min<int64_t>(cap, m.ne11 - c0);
        const uint16_t * x = xb + c0 * m.K;
        float * d = (float *) ((char *) m.dst + c0 * m.nb1);
        switch (nc) {
            case 1: launch_gemv<1>(m, x, d, s); break;
            case 2: launch_gemv<2>(m, x, d, s); break;
            case 3: launch_gemv<3>(m, x, d, s); break;
            case 4: launch_gemv<4>(m, x, d, s); break;
            case 5: launch_gemv<5>(m, x, d, s); break;
            case 6: launch_gemv<6>(m, x, d, s); break;
            case 7: launch_gemv<7>(m, x, d, s); break;
            default: launch_gemv<8>(m, x, d, s); break;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// prompts, tree order
// ---------------------------------------------------------------------------------------------

// 32 weight rows x 32 prompt columns per workgroup; wave w the 64-deep K chunks w, w + 4, ... Both
// operands are loaded coalesced (8 lanes per 128-byte row segment, 8 rows per instruction; a piece past
// K is zeroed, a row past N or a column past ncols re-reads the last one) into wave-private LDS tiles of
// row stride 144 B, from which lane l reads the fragment of row / column l % 32, k = 8 (l / 32) + j of each
// 16-deep step. The next chunk's loads are in flight while the current one is multiplied. The partial
// tiles meet in LDS and are added in wave order. K % 8 == 0, 16-byte aligned rows.
__global__ __launch_bounds__(256, 2) void k_mm_bf16p(const uint8_t * __restrict__ W, size_t nb01, int64_t K, int64_t N,
                                                     const uint16_t * __restrict__ xb, int64_t ncols, float * __restrict__ dst,
                                                     size_t ycol) {
    constexpr int kRow = 72;  // bf16 per LDS row (64 + 8 pad)
    constexpr int NW = 4;
    __shared__ __attribute__((aligned(16))) uint16_t lw[NW][32 * kRow];
    __shared__ __attribute__((aligned(16))) uint16_t lx[NW][32 * kRow];
    __shared__ __attribute__((aligned(16))) float red[NW][16][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int lr = lane >> 3, lp = lane & 7;  // staging: row lr + 8 q, 16-byte piece lp
    const int64_t nrt = (N + 31) / 32;
    const int64_t n0 = ((int64_t) blockIdx.x % nrt) * 32, c0 = ((int64_t) blockIdx.x / nrt) * 32;
    const int nch = (int) ((K + 63) / 64);  // 64-deep chunks, the last one ragged
    const uint8_t * wq[4];
    const uint8_t * xq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        wq[q] = W + std::min<int64_t>(n0 + lr + 8 * q, N - 1) * nb01;
        xq[q] = (const uint8_t *) (xb + std::min<int64_t>(c0 + lr + 8 * q, ncols - 1) * K);
    }
    struct Chunk {
        u32x4 wv[4];
        u32x4 xv[4];
    };
    auto load = [&](Chunk & c, int i) {
        i = i < nch ? i : nch - 1;  // past the end: a harmless re-read of the last chunk
        const int64_t k = (int64_t) i * 64 + 8 * lp;
        const bool in = k < K;
        const size_t off = (size_t) (in ? k : 0) * 2;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            c.wv[q] = *(const u32x4 *) (wq[q] + off);
            c.xv[q] = *(const u32x4 *) (xq[q] + off);
            if (!in) c.wv[q] = (u32x4) (0u);
            if (!in) c.xv[q] = (u32x4) (0u);
        }
    };
    uint16_t * tw = lw[w];
    uint16_t * tx = lx[w];
    float16v acc = {};
    auto step = [&](const Chunk & c) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            *(u32x4 *) (tw + (lr + 8 * q) * kRow + 8 * lp) = c.wv[q];
            *(u32x4 *) (tx + (lr + 8 * q) * kRow + 8 * lp) = c.xv[q];
        }
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const u32x4 a = *(const u32x4 *) (tw + r * kRow + 16 * st + 8 * h);
            const u32x4 b = *(const u32x4 *) (tx + r * kRow + 16 * st + 8 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
        }
    };
    // (LDS operations of one wave execute in order: one buffer per operand suffices)
    Chunk cur, nxt;
    if (w < nch) load(cur, w);
    for (int i = w; i < nch; i += NW) {  // wave-uniform bounds
        load(nxt, i + NW);
        step(cur);
        cur = nxt;
    }
#pragma unroll
    for (int el = 0; el < 16; el++) red[w][el][lane] = acc[el];
    __syncthreads();
    // wave w stores accumulator elements 4w .. 4w + 3 (rows n0 + 8 w + 4 (l / 32) + e) of column c0 + l % 32
    const int64_t b = c0 + r;
    const int64_t n = n0 + 8 * w + 4 * h;
    if (b >= ncols) return;
    float * out = (float *) ((char *) dst + b * ycol);
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int el = 4 * w + e;
        const float y = ((red[0][el][lane] + red[1][el][lane]) + red[2][el][lane]) + red[3][el][lane];
        if (n + e < N) out[n + e] = y;
    }
}

bool prompt_supported(const mi_mm_desc & m, const uint16_t * xb) {
    return !m.id.ids && m.ne02 == 1 && m.ne03 == 1 && m.ne12 == 1 && m.ne13 == 1 && m.ne11 > 8 && rows_aligned(m, xb) && m.N >= 1 &&
           ((m.N + 31) / 32) * ((m.ne11 + 31) / 32) <= INT32_MAX;
}

} // namespace

void mi_convert_bf16(const mi_src_cols & x, int64_t K, uint16_t * out, int src_type, hipStream_t s) {
    const int64_t ncols = x.ne1 * x.ne2 * x.ne3;
    if (ncols == 0 || K == 0) return;
    const dim3 grid((unsigned) ncols, (unsigned) std::min<int64_t>((K + 255) / 256, 64));
    if (src_type == MI_TYPE_BF16) hipLaunchKernelGGL(k_convert_bf16<MI_TYPE_BF16>, grid, dim3(256), 0, s, x, K, out);
    else if (src_type == MI_TYPE_F16) hipLaunchKernelGGL(k_convert_bf16<MI_TYPE_F16>, grid, dim3(256), 0, s, x, K, out);
    else if (src_type == MI_TYPE_F32) hipLaunchKernelGGL(k_convert_bf16<MI_TYPE_F32>, grid, dim3(256), 0, s, x, K, out);
    else MI_ASSERT(!"mi_convert_bf16: src1 must be F32, F16 or BF16");
}

void mi_mul_mat_bf16(const mi_mm_desc & m, const uint16_t * xb, hipStream_t s) {
    MI_ASSERT(m.type == MI_TYPE_BF16);
    if (m.N == 0 || m.ne11 * m.ne12 * m.ne13 == 0) return;
    if (mi_mmv_order() != 1 && gemv_supported(m, xb)) {
        mul_mat_gemv(m, xb, s);
    } else if (mi_mmv_order() != 1 && prompt_supported(m, xb)) {
        const int64_t tiles = ((m.N + 31) / 32) * ((m.ne11 + 31) / 32);
        hipLaunchKernelGGL(k_mm_bf16p, dim3((unsigned) tiles), dim3(256), 0, s, (const uint8_t *) m.W, m.nb01, m.K, m.N, xb, m.ne11, m.dst, m.nb1);
    } else {
        mul_mat_ord(m, xb, s);
    }
}
