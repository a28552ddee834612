// mmq.hip -- batched GGML_OP_MUL_MAT (prompt / prefill regime, more than 8 activation columns) for
// F16 weights on the gfx950 matrix cores (v_mfma_f32_32x32x16_f16).
//
// Activations: the f16-rounded columns of ggml_fp32_to_fp16_row, as the CPU uses them, written once
// by mi_convert_f16 in the K-blocked layout [K/16][ncols][16]: a 16-deep K step of 32 columns is 1 KB
// contiguous, one 16-byte load per lane straight into an MFMA operand register.
//
// k_mmq3 (more than 128 columns): 64 weight rows x 128 columns per workgroup, each wave all 64 rows x
// its own 32 columns; only the weight slab passes through LDS. 4096 x 4096, B = 512: 43 us (395
// TFLOP/s). (Its predecessor staged row-major activations through LDS as well: 53 us, removed.
// An XCD-contiguous tile order for k_mmq3 never beat the plain grid: removed.)
// k_mmf16p (9..128 columns): 32 x 32 tiles with K split over the tile's 4 waves, so that a short
// prompt still fills the chip.
//
// Products of fp16 values are exact in f32: against the CPU only the f32 summation order differs.
// Roofline: 2*N*K*B flops against 2*N*K + 2*K*B + 4*N*B bytes -- at B=512, N=K=4096 ~17.2 GFLOP over
// ~46 MB: MFMA-bound (f16 dense ~2.5 PF/s).
// (Quantized weights once ran here too, dequantized to f16 against f16(d * q) activations -- about
// 2^-11 per operand; the exact int8 GEMMs of mmq_exact.hip replaced that path: removed.)

#include <algorithm>

#include "mi355x_common.h"
#include "mi355x_kernels.h"

namespace {

constexpr int BM = 64;          // weight rows per tile
constexpr int BN = 128;         // activation columns per tile
constexpr int BK = 64;          // K per LDS stage
constexpr int LDS_STRIDE = BK + 8;  // padded f16 row stride (144 B)
constexpr int kPF = 4;          // stages of global loads in flight (register ring)

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

// raw loads for 16 consecutive f16 weights of one row (loaded before a stage's MFMAs, stored to LDS
// after them)
struct WRawF16 {
    uint4 a, b;
    __device__ __forceinline__ void load(const uint8_t * row, int64_t k) {
        a = *(const uint4 *) (row + k * 2);
        b = *(const uint4 *) (row + k * 2 + 16);
    }
};

// ---- k_mmq3: activations straight into MFMA operand registers ------------------------------------
// A 64 x 128 workgroup tile with K split over SK groups of 4 waves. Each wave owns all 64 weight
// rows x its own 32 activation columns: the f16 activation fragment of a 16-deep K step is one
// 16-byte load per lane straight from xh (lane l: column l & 31, k + 8 (l >> 5)), held in a
// register ring kPF stages deep, so activations never pass through LDS (staging them there left the
// LDS array, not the MFMAs, as the busiest unit). Only the 64 x 64 weight slab of a stage goes
// through LDS, written once per group and read by its four waves (two A fragments per K step each).
// NST: the K stages per group as a compile-time constant (0: K / BK / SK at run time).
template <int SK, int NST>
__global__ __launch_bounds__(256 * SK) void k_mmq3(const uint8_t * __restrict__ W, size_t nb01, int64_t K, int64_t N,
                                              const uint16_t * __restrict__ xh, int64_t ncols, float * __restrict__ dst,
                                              size_t ycol) {
    constexpr int kSlab = 2 * BM * LDS_STRIDE;  // halves per group: double-buffered weight slab
    constexpr int kRedBytes = 256 * 32 * 4;     // one group's partial tile (SK == 2 hand-off)
    constexpr int kSlabBytes = SK * kSlab * 2;
    __shared__ __attribute__((aligned(16))) char lds_raw[SK == 2 && kRedBytes > kSlabBytes ? kRedBytes : kSlabBytes];
    using Raw = WRawF16;
    const int grp = (int) threadIdx.x >> 8;
    const int tid = (int) threadIdx.x & 255;
    _Float16 * la0 = (_Float16 *) lds_raw + grp * kSlab;
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t n0 = (int64_t) blockIdx.x * BM;
    const int64_t b0 = (int64_t) blockIdx.y * BN;

    // weight staging: thread t copies row t/4, 16 elements at (t%4)*16
    const int ar = tid >> 2, ak = (tid & 3) * 16;
    const int64_t arow = n0 + ar;
    const bool alive = arow < N;
    const uint8_t * wrow = W + (alive ? arow : 0) * nb01;
    // activation fragment: column b0 + 32 wave + (lane & 31), 8 halves at k + 8 (lane >> 5), from
    // the K-blocked layout xh[k / 16][ncols][16]: one K step of 32 columns = 1 KB contiguous
    const int64_t bcol = std::min<int64_t>(b0 + 32 * wave + (lane & 31), ncols - 1);
    const uint16_t * xcol = xh + bcol * 16 + 8 * (lane >> 5);
    const int64_t kstep = ncols * 16;  // halves per 16-deep K step

    Raw raw[kPF];
    half8 xb[kPF][BK / 16];
    auto load_stage = [&](Raw & rw, half8 (&xv)[BK / 16], int64_t k0) {
        rw.load(wrow, k0 + ak);
#pragma unroll
        for (int i = 0; i < BK / 16; i++) xv[i] = *(const half8 *) (xcol + (k0 / 16 + i) * kstep);
    };
    auto store_stage = [&](int buf, const Raw & rw) {
        _Float16 * pa = la0 + buf * (BM * LDS_STRIDE) + ar * LDS_STRIDE + ak;
        *(uint4 *) pa = alive ? rw.a : make_uint4(0, 0, 0, 0);
        *(uint4 *) (pa + 8) = alive ? rw.b : make_uint4(0, 0, 0, 0);
    };

    float16v acc0 = {}, acc1 = {};  // rows 0..31 / 32..63 of the tile, this wave's 32 columns
    const int r = lane & 31, h = lane >> 5;
    const int64_t nst = NST ? NST : K / BK / SK;
    const int64_t kg = (int64_t) grp * nst * BK;
#pragma unroll
    for (int u = 0; u < kPF; u++) load_stage(raw[u], xb[u], kg + (int64_t) (u < nst ? u : nst - 1) * BK);
    store_stage(0, raw[0]);
    mi_lds_barrier();
#pragma unroll (NST ? NST / kPF : 1)
    for (int64_t s0 = 0; s0 < nst; s0 += kPF) {
#pragma unroll
        for (int u = 0; u < kPF; u++) {
            const int64_t st = s0 + u;
            const int cur = (int) (st & 1);
            const _Float16 * pa0 = la0 + cur * (BM * LDS_STRIDE) + r * LDS_STRIDE + 8 * h;
            const _Float16 * pa1 = pa0 + 32 * LDS_STRIDE;
            // all of the stage's A fragments are requested before the first MFMA, so the LDS
            // latency is exposed once per stage rather than once per K step
            half8 a0[BK / 16], a1[BK / 16];
#pragma unroll
            for (int kk = 0; kk < BK / 16; kk++) {
                a0[kk] = *(const half8 *) (pa0 + 16 * kk);
                a1[kk] = *(const half8 *) (pa1 + 16 * kk);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < BK / 16; kk++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[kk], xb[u][kk], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[kk], xb[u][kk], acc1, 0, 0, 0);
            }
            const int un = (u + 1) % kPF;
            store_stage(cur ^ 1, raw[un]);  // last: a harmless rewrite (the ring's loads are clamped to the last stage)
            // slot u's activations are consumed and its weights are in LDS: refill with st + kPF
            const int64_t nxt = st + kPF < nst ? st + kPF : nst - 1;
            load_stage(raw[u], xb[u], kg + nxt * BK);
            mi_lds_barrier();  // keeps the ring's global loads in flight
        }
    }

    if constexpr (SK == 2) {
        // group 1 hands its partial tile to group 0 through LDS (the slabs are idle once every
        // wave is past its last MFMA); the sum is group0 + group1 in that fixed order
        float * red = (float *) lds_raw;
        __syncthreads();
        if (grp == 1) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                red[(i * 2 + 0) * 256 + tid] = acc0[i];
                red[(i * 2 + 1) * 256 + tid] = acc1[i];
            }
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            acc0[i] += red[(i * 2 + 0) * 256 + tid];
            acc1[i] += red[(i * 2 + 1) * 256 + tid];
        }
    }

    // D[n][b]: column b = lane & 31 of this wave's 32, rows n = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    const int64_t b = b0 + 32 * wave + (lane & 31);
    if (b >= ncols) return;
    float * out = (float *) ((char *) dst + b * ycol);
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const float16v & acc = half ? acc1 : acc0;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int64_t n = n0 + 32 * half + 8 * g + 4 * (lane >> 5);
            if (n + 3 < N) {
                *(float4 *) (out + n) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) if (n + e < N) out[n + e] = acc[4 * g + e];
            }
        }
    }
}

// ---- F16 weights, short prompts (<= 128 columns): 32 x 32 tiles, K split over the 4 waves -------
// k_mmq3's 64 x 128 tiles give N / 64 workgroups at B <= 128 (64 of the 256 CUs at N = 4096). Here
// a workgroup computes 32 weight rows x 32 prompt columns and wave w the K range [w K/4, (w+1) K/4)
// on v_mfma_f32_32x32x16_f16, 64 K per chunk, a register ring PF chunks deep:
//  * weights: coalesced loads (8 lanes per 128-byte row segment, 8 rows per instruction) into a
//    wave-private LDS tile (row stride 144 B: the MFMA fragment reads of 16 rows hit 16 distinct
//    bank quads), then one ds_read_b128 per lane and K step (row lane % 32, halves 8 (lane / 32));
//    LDS operations of one wave execute in order, so one buffer suffices;
//  * activations: the K-blocked f16 layout [K/16][ncols][16] -- a 16-deep step of 32 columns is 1 KB
//    contiguous, one 16-byte load per lane.
// (A first version loaded both operands row-per-lane straight from global memory: every lane
// touched its own cache line, TCP_TOTAL_CACHE_ACCESSES = 64 per load instruction, 19.5 us at B = 64,
// profiles/r03z_f16_pmc.txt.) The four partial tiles meet in LDS and are added in wave order.
// Products of fp16 values are exact in f32; only the summation order differs from the reference's
// ggml_vec_dot_f16 (~1e-7 relative).
template <int PF>
__global__ __launch_bounds__(256, 2) void k_mmf16p(const uint8_t * __restrict__ W, size_t nb01, int64_t K, int64_t N,
                                                   const uint16_t * __restrict__ xh, int64_t ncols, float * __restrict__ dst,
                                                   size_t ycol) {
    constexpr int NW = 4;     // waves per tile (8, K in eighths, measured slower: profiles/r03aa_prefill_f16_8wave.txt, removed)
    constexpr int kRow = 72;  // halves per LDS row (64 + 8 pad)
    __shared__ __attribute__((aligned(16))) _Float16 lw[NW][32 * kRow];
    __shared__ __attribute__((aligned(16))) float red[NW][16][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int lr = lane >> 3, lp = lane & 7;  // weight staging: row lr + 8 q, 16-byte piece lp
    const int64_t nrt = (N + 31) / 32;
    const int64_t n0 = ((int64_t) blockIdx.x % nrt) * 32, c0 = ((int64_t) blockIdx.x / nrt) * 32;
    const int64_t kw = K / NW;       // this wave's K range (K % (64 NW) == 0)
    const int nch = (int) (kw / 64);  // 64-deep chunks
    const uint8_t * wq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) wq[q] = W + std::min<int64_t>(n0 + lr + 8 * q, N - 1) * nb01 + (size_t) (w * kw) * 2 + 16 * lp;
    const int64_t col = std::min<int64_t>(c0 + r, ncols - 1);
    const uint16_t * xc = xh + ((size_t) (w * kw / 16) * ncols + col) * 16 + 8 * h;
    const size_t xstep = (size_t) ncols * 16;  // halves per 16-deep K step
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // (a HIP uint4 array is not promoted to registers)
    struct Chunk {
        u32x4 wv[4];
        u32x4 xv[4];
    };
    auto load = [&](Chunk & c, int i) {
        i = i < nch ? i : nch - 1;  // past the end: a harmless re-read of the last chunk
#pragma unroll
        for (int q = 0; q < 4; q++) c.wv[q] = *(const u32x4 *) (wq[q] + (size_t) i * 128);
#pragma unroll
        for (int st = 0; st < 4; st++) c.xv[st] = *(const u32x4 *) (xc + ((size_t) i * 4 + st) * xstep);
    };
    _Float16 * tile = lw[w];
    Chunk ring[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) load(ring[u], u);
    float16v acc = {};
    auto step = [&](Chunk & c, int i) {
        if (i >= nch) return;  // uniform
#pragma unroll
        for (int q = 0; q < 4; q++) *(u32x4 *) (tile + (lr + 8 * q) * kRow + 8 * lp) = c.wv[q];
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const half8 a = *(const half8 *) (tile + r * kRow + 16 * st + 8 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(half8, c.xv[st]), acc, 0, 0, 0);
        }
        load(c, i + PF);
    };
    static_assert(PF == 2 || PF == 3, "the ring below is written out for 2 or 3 chunks");
    for (int i0 = 0; i0 < nch; i0 += PF) {  // ring slots named statically (no private-array indexing)
        step(ring[0], i0);
        step(ring[1], i0 + 1);
        if constexpr (PF == 3) step(ring[PF - 1], i0 + 2);
    }
#pragma unroll
    for (int el = 0; el < 16; el++) red[w][el][lane] = acc[el];
    __syncthreads();
    // wave w stores accumulator elements 4w .. 4w + 3 (rows n0 + 8 w + 4 (l / 32) + e) of column
    // c0 + l % 32, the NW partial tiles added in wave order
    const int64_t b = c0 + r;
    const int64_t n = n0 + 8 * w + 4 * h;
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int el = 4 * w + e;
        y[e] = red[0][el][lane] + red[1][el][lane];
#pragma unroll
        for (int v = 2; v < NW; v++) y[e] = y[e] + red[v][el][lane];
    }
    if (b >= ncols) return;
    float * out = (float *) ((char *) dst + b * ycol);
    if (n + 3 < N) {
        *(float4 *) (out + n) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) if (n + e < N) out[n + e] = y[e];
    }
}

} // namespace

bool mi_mmf16p_supported(int64_t K, int64_t N, size_t nb01, int64_t ncols, size_t ycol) {
    return ncols > 8 && ncols <= 128 && K % 256 == 0 && N >= 1 && nb01 % 16 == 0 && ycol % 16 == 0;
}

void mi_mul_mat_f16p(const void * W, size_t nb01, int64_t K, int64_t N, const uint16_t * xh, int64_t ncols, float * dst, size_t ycol,
                     hipStream_t s) {
    const int64_t tiles = ((N + 31) / 32) * ((ncols + 31) / 32);
    mi_route("k_mmf16p<pf3>");
    hipLaunchKernelGGL((k_mmf16p<3>), dim3((unsigned) tiles), dim3(256), 0, s, (const uint8_t *) W, nb01, K, N, xh, ncols, dst, ycol);
}

bool mi_mmq_supported(int64_t K, size_t nb01, size_t ycol) { return K % 256 == 0 && nb01 % 16 == 0 && ycol % 16 == 0; }

void mi_mul_mat_mmq(const void * W, size_t nb01, int64_t K, int64_t N, const uint16_t * xh, int64_t ncols, float * dst, size_t ycol,
                    hipStream_t s) {
    const dim3 grid((unsigned) ((N + BM - 1) / BM), (unsigned) ((ncols + BN - 1) / BN));
    const uint8_t * w = (const uint8_t *) W;
    // split K over two 4-wave groups when each group keeps a whole number of ring turns: with
    // one 64x128 tile per CU (grid <= 256) a single 4-wave group leaves one wave per SIMD.
    // k_mmq3 is fully unrolled over the K stages for the common K (the loop back-edge of the
    // runtime-K loop makes the compiler drain the load ring: measured 47 -> 43 us at 4096)
    const bool sk2 = K % (2 * BK * kPF) == 0;
    const int nst2 = sk2 ? (int) (K / BK / 2) : 0;
#define MI_MMQ3(SK, NST) do { mi_route("k_mmq3<sk" #SK ",nst" #NST ">"); \
        hipLaunchKernelGGL((k_mmq3<SK, NST>), grid, dim3(256 * SK), 0, s, w, nb01, K, N, xh, ncols, dst, ycol); } while (0)
    if (nst2 == 32) MI_MMQ3(2, 32);
    else if (nst2 == 24) MI_MMQ3(2, 24);
    else if (nst2 == 16) MI_MMQ3(2, 16);
    else if (sk2) MI_MMQ3(2, 0);
    else MI_MMQ3(1, 0);
#undef MI_MMQ3
}
