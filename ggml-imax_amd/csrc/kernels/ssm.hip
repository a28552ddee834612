// ssm.hip -- the two state-space ops of a Mamba layer on gfx950, written from the reference CPU forwards
// (the reference has no device kernel for either):
//   ssm_conv   src/ggml.c:16311-16418   the rolling 1-D convolution over the conv state -- the CPU's bits
//   ssm_scan   src/ggml.c:16437-16543   the selective scan -- expf / log1pf to 1 ulp, not the CPU's bits
//
// Both write a 1-D dst: the outputs [d_inner, n_tokens], then the new states of all n_kv sequences. Rows
// (d_inner) are independent and tokens are sequential, so a row belongs to one lane (conv, generic scan)
// or to 16 lanes (scan with d_state 16), the token loop runs inside the kernel, and everything a row
// writes -- the copies into other sequences' states too -- is written by the lanes that own it: no
// ordering between workgroups is needed and any n_tokens / n_kv is one launch.
//
// Sequences. sq [n_kv, n_tokens] i32 is read here, on the device. Token t works on the state of sequence
// sq[0, t]: it reads it (from src for the first token, from dst afterwards), updates it, writes it to
// dst and copies it to the states sq[1, t], sq[2, t], .. up to the first id outside [0, n_kv). With
// n_kv > 1 the reference first copies every state from src to dst, so "from src for the first token" and
// "from dst" read the same values; the kernels make that copy too, then keep the state of the current
// sequence in registers for as long as consecutive tokens stay on it, and store it when the sequence
// changes and at the end. A token whose sq[0] is outside [0, n_kv) (the CPU aborts) is skipped whole:
// no state moves and its output is not written.

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#pragma clang fp contract(off)

namespace {

struct ssm_conv_args {
    const char * s;    // [d_conv - 1, d_inner, n_kv], rows contiguous
    const char * x;    // [d_inner, n_t], nb0 == 4
    const float * c;   // [d_conv, d_inner] contiguous
    const char * sq;   // [n_kv, n_t] i32, nb0 == 4
    float * dst;
    int d_inner, n_t, n_kv;
    size_t s_nb2, x_nb1, sq_nb1;
};

struct ssm_scan_args {
    const float * s;   // [d_state, d_inner, n_kv] contiguous
    const float * x;   // [d_inner, n_t] contiguous
    const char * dt;   // [d_inner, n_t], nb0 == 4
    const char * A;    // [d_state, d_inner], nb0 == 4
    const char * B;    // [d_state, n_t], nb0 == 4
    const char * C;
    const char * sq;   // [n_kv, n_t] i32, nb0 == 4
    float * dst;
    int d_state, d_inner, n_t, n_kv;
    size_t dt_nb1, A_nb1, B_nb1, C_nb1, sq_nb1;
};

__device__ __forceinline__ const int32_t * sq_row(const char * sq, size_t nb1, int t) {
    return (const int32_t *) (sq + (size_t) t * nb1);
}

// ---- ssm_conv: one lane per row, the d_conv state values of the current sequence in registers ------------
// The dot is the reference's `sumf += s[i] * c[i]` from 0.0f in column order as its gcc -O3 -mfma build
// rounds it: gcc vectorizes the loop four columns at a time -- a vector multiply, then the four products
// added to sumf one by one, nothing fused -- and contracts only the scalar remainder loop into fmaf. So the
// first 4 * (d_conv / 4) terms are a rounded product plus a rounded sum and the rest fmaf(s, c, sumf)
// (d_conv 4: no fmaf at all; d_conv 3: all fmaf). Identified from the reference build's outputs for
// d_conv 2 .. 13 (tests/test_ssm.py::test_reference_conv_rounding_sequence holds it in place).
//
// Tokens are taken kConvGroup at a time: the group's x values and what its sq rows say are loaded before the
// previous group is worked on (nothing on the chain waits for memory), and a group whose tokens are all
// valid, on one sequence and copy nowhere -- every group of a single-sequence batch -- runs as straight-line
// code. Any other group goes token by token through the sequence handling.
constexpr int kConvBlock = 64;
constexpr int kConvGroup = 16;

// the x values of row r for tokens t0 .. t0 + kConvGroup - 1, and in `same` the sequence all of them work
// on, or -1: a token past the end, an id outside [0, n_kv), a change of sequence or a copy. Every load is
// issued before any is looked at (tokens past the end are clamped to the last one: loaded, never used).
__device__ __forceinline__ void conv_load(const ssm_conv_args & a, int r, int t0, float (&xv)[kConvGroup], int & same) {
    same = -1;
    if (t0 >= a.n_t) {
#pragma unroll
        for (int j = 0; j < kConvGroup; j++) xv[j] = 0.0f;
        return;
    }
    int s0[kConvGroup], s1[kConvGroup];
#pragma unroll
    for (int j = 0; j < kConvGroup; j++) {
        const int t = min(t0 + j, a.n_t - 1);
        xv[j] = *(const float *) (a.x + (size_t) t * a.x_nb1 + (size_t) r * sizeof(float));
        s0[j] = sq_row(a.sq, a.sq_nb1, t)[0];
        s1[j] = -1;
    }
    if (a.n_kv > 1) {
#pragma unroll
        for (int j = 0; j < kConvGroup; j++) s1[j] = sq_row(a.sq, a.sq_nb1, min(t0 + j, a.n_t - 1))[1];
    }
#pragma unroll
    for (int j = 0; j < kConvGroup; j++) {
        const bool alone = (t0 + j < a.n_t) & (s0[j] >= 0) & (s0[j] < a.n_kv) & !((s1[j] >= 0) & (s1[j] < a.n_kv));
        const int s = alone ? s0[j] : -1;
        same = j == 0 || s == same ? s : -1;
    }
    same = __builtin_amdgcn_readfirstlane(same);  // the same in every lane: a scalar branch
}

template <int NC>
__device__ __forceinline__ float conv_dot(const float (&st)[NC], const float (&cw)[NC]) {
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < NC; i++) sum = i < (NC & ~3) ? sum + st[i] * cw[i] : __builtin_fmaf(st[i], cw[i], sum);
    return sum;
}

template <int NC>
__global__ __launch_bounds__(kConvBlock) void k_ssm_conv(ssm_conv_args a) {
    const int r = blockIdx.x * kConvBlock + threadIdx.x;
    if (r >= a.d_inner) return;
    float * out = a.dst;
    float * ds = a.dst + (size_t) a.d_inner * a.n_t;  // [NC, d_inner, n_kv]
    const size_t seq = (size_t) NC * a.d_inner;
    float cw[NC], st[NC];
#pragma unroll
    for (int i = 0; i < NC; i++) {
        cw[i] = a.c[(size_t) r * NC + i];
        st[i] = 0.0f;
    }
    if (a.n_kv > 1) {
        for (int i3 = 0; i3 < a.n_kv; i3++) {
            const float * s0 = (const float *) (a.s + (size_t) i3 * a.s_nb2) + (size_t) r * (NC - 1);
#pragma unroll
            for (int i = 0; i < NC - 1; i++) ds[i3 * seq + (size_t) r * NC + 1 + i] = s0[i];
        }
    }
    int cur = -1;
    // the state of sequence s0 into the registers (the one held goes to dst first)
    auto take = [&](int s0) {
        if (cur >= 0) {
#pragma unroll
            for (int i = 0; i < NC; i++) ds[cur * seq + (size_t) r * NC + i] = st[i];
        }
        // columns 1 .. of the dst state (the copy above), or the src state itself
        const float * from = a.n_kv > 1 ? ds + s0 * seq + (size_t) r * NC + 1
                                        : (const float *) (a.s + (size_t) s0 * a.s_nb2) + (size_t) r * (NC - 1);
#pragma unroll
        for (int i = 0; i < NC - 1; i++) st[1 + i] = from[i];
        cur = s0;
    };
    float xv[kConvGroup], xn[kConvGroup];
    int same, same_n;
    conv_load(a, r, 0, xv, same);
    for (int t0 = 0; t0 < a.n_t; t0 += kConvGroup) {
        conv_load(a, r, t0 + kConvGroup, xn, same_n);  // (past the end: no loads)
        if (same >= 0) {
            if (same != cur) take(same);
#pragma unroll
            for (int j = 0; j < kConvGroup; j++) {
#pragma unroll
                for (int i = 0; i < NC - 1; i++) st[i] = st[i + 1];
                st[NC - 1] = xv[j];
                out[(size_t) (t0 + j) * a.d_inner + r] = conv_dot<NC>(st, cw);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kConvGroup; j++) {
                const int t = t0 + j;
                if (t >= a.n_t) break;
                const int32_t * sq = sq_row(a.sq, a.sq_nb1, t);
                const int s0 = sq[0];
                if (s0 < 0 || s0 >= a.n_kv) continue;
                if (s0 != cur) take(s0);
#pragma unroll
                for (int i = 0; i < NC - 1; i++) st[i] = st[i + 1];
                st[NC - 1] = xv[j];
                for (int i3 = 1; i3 < a.n_kv; i3++) {
                    const int to = sq[i3];
                    if (to < 0 || to >= a.n_kv) break;
#pragma unroll
                    for (int i = 0; i < NC; i++) ds[to * seq + (size_t) r * NC + i] = st[i];
                }
                out[(size_t) t * a.d_inner + r] = conv_dot<NC>(st, cw);
            }
        }
#pragma unroll
        for (int j = 0; j < kConvGroup; j++) xv[j] = xn[j];
        same = same_n;
    }
    if (cur >= 0) {
#pragma unroll
        for (int i = 0; i < NC; i++) ds[cur * seq + (size_t) r * NC + i] = st[i];
    }
}

// ---- ssm_scan, d_state 16: lane = (row, state element), 16 rows per workgroup of 256 -----------------------
// Per chunk of kScanChunk tokens the workgroup stages, in LDS, what does not depend on the state:
//   dx[t][row] = {dtsp, x * dtsp} with dtsp = dt <= 20 ? log1pf(expf(dt)) : dt   (once per row and token,
//                                                                                  not once per lane)
//   bc[t][n]   = {B, C}
//   same[g]    = the sequence of the chunk's g-th group of kScanGroup tokens when they are all valid, on one
//                sequence and copy nowhere (every full group of a single-sequence batch), else -1
// Then each lane walks the chunk a group at a time. A group with same[g] >= 0 is straight-line code: dA =
// expf(dtsp * A) and dBx = B * (x * dtsp) of its kScanGroup tokens, independent of each other and of the
// state, then the chain state = fmaf(state, dA, dBx) and y = the sum over the row's 16 lanes of state * C
// (DPP, a tree order) -- only the fmaf is sequential, the rest overlaps across tokens. Any other group
// (a change of sequence, a copy, a skipped token, the ragged end) goes token by token through the
// sequence handling. y goes to LDS and leaves in 64-byte row segments per token. The global loads of the
// next chunk are issued before the chain of the current one and land in registers while it runs.
constexpr int kScanRows = 16;
constexpr int kScanChunk = 64;
constexpr int kScanGroup = 8;
static_assert(kScanChunk % kScanGroup == 0 && kScanGroup <= 16, "whole groups; lane n stores the y of the group's n-th token");

__device__ __forceinline__ float row16_sum(float v) {  // the sum over each aligned group of 16 lanes, in every lane
    auto f = [](int x) { return __int_as_float(x); };
    auto i = [](float x) { return __float_as_int(x); };
    v += f(mi_dpp<MI_DPP_QP_1032>(0, i(v)));
    v += f(mi_dpp<MI_DPP_QP_2301>(0, i(v)));
    v += f(mi_dpp<MI_DPP_ROW_HALF_MIRROR>(0, i(v)));
    v += f(mi_dpp<MI_DPP_ROW_MIRROR>(0, i(v)));
    return v;
}

static_assert(kScanChunk == MI_WAVE, "the first wave holds a chunk's ids one token per lane");

__device__ __forceinline__ float softplus_ref(float dt) {
    const float sp = log1pf(expf(dt));  // (computed either way: a select, no branch; inf for a large dt, not taken)
    return dt <= 20.0f ? sp : dt;
}

template <bool MULTI>
__global__ __launch_bounds__(kScanRows * 16) void k_ssm_scan16(ssm_scan_args a) {
    __shared__ float2 dx[kScanChunk][kScanRows];
    __shared__ float2 bc[kScanChunk][16];
    __shared__ float ys[kScanChunk][kScanRows];
    __shared__ int sq0[kScanChunk];  // sq[0, t], or -1: skip the token
    __shared__ int same[kScanChunk / kScanGroup];

    const int tid = threadIdx.x;
    const int rl = tid >> 4, n = tid & 15;
    const int row0 = blockIdx.x * kScanRows;
    const int row = row0 + rl;
    const bool valid = row < a.d_inner;
    float * ds = a.dst + (size_t) a.d_inner * a.n_t;  // [16, d_inner, n_kv]
    const size_t seq = (size_t) 16 * a.d_inner;
    const size_t mine = (size_t) row * 16 + n;
    const float An = valid ? *(const float *) (a.A + (size_t) row * a.A_nb1 + n * sizeof(float)) : 0.0f;
    if (MULTI && valid) {
        for (int i3 = 0; i3 < a.n_kv; i3++) ds[i3 * seq + mine] = a.s[i3 * seq + mine];
    }
    const float * from = MULTI ? ds : a.s;
    float state = 0.0f;
    int cur = -1;

    // A chunk's inputs as this thread loads them: kPer (token, element) pairs of dt, x, B, C and, in the first
    // wave, the ids of token `tid`. Tokens and rows past the end are clamped to the last one: loaded without
    // a branch, never used. The loads of chunk c + 1 are issued before the chain of chunk c runs.
    constexpr int kPer = kScanChunk * 16 / (kScanRows * 16);
    float in_dt[kPer], in_x[kPer], in_b[kPer], in_c[kPer];
    int in_s0 = -1, in_s1 = -1;
    auto load_chunk = [&](int t0) {
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int idx = tid + k * kScanRows * 16;
            const int t = min(t0 + (idx >> 4), a.n_t - 1), e = idx & 15;
            const int rc = min(row0 + e, a.d_inner - 1);
            in_dt[k] = *(const float *) (a.dt + (size_t) t * a.dt_nb1 + (size_t) rc * sizeof(float));
            in_x[k] = a.x[(size_t) t * a.d_inner + rc];
            in_b[k] = *(const float *) (a.B + (size_t) t * a.B_nb1 + e * sizeof(float));
            in_c[k] = *(const float *) (a.C + (size_t) t * a.C_nb1 + e * sizeof(float));
        }
        if (tid < kScanChunk) {
            const int32_t * sq = sq_row(a.sq, a.sq_nb1, min(t0 + tid, a.n_t - 1));
            in_s0 = sq[0];
            if (MULTI) in_s1 = sq[1];
        }
    };
    if (a.n_t > 0) load_chunk(0);

    for (int t0 = 0; t0 < a.n_t; t0 += kScanChunk) {
        const int nt = min(kScanChunk, a.n_t - t0);
        // ---- stage the chunk
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int idx = tid + k * kScanRows * 16;
            if ((idx >> 4) >= nt) break;  // (a decode step stages one token, not kScanChunk copies of it)
            const float sp = softplus_ref(in_dt[k]);
            dx[idx >> 4][idx & 15] = make_float2(sp, in_x[k] * sp);
            bc[idx >> 4][idx & 15] = make_float2(in_b[k], in_c[k]);
        }
        if (tid < kScanChunk) {  // the first wave, whole: lane = token
            const int s0 = tid < nt && in_s0 >= 0 && in_s0 < a.n_kv ? in_s0 : -1;
            sq0[tid] = s0;
            const int alone = MULTI && in_s1 >= 0 && in_s1 < a.n_kv ? -1 : s0;  // -1: skipped, or it copies its state
            const int lead = __shfl(alone, tid & ~(kScanGroup - 1), MI_WAVE);
            const unsigned long long ok = __ballot(alone >= 0 && alone == lead);
            constexpr unsigned long long kAll = (1ull << kScanGroup) - 1;
            if ((tid & (kScanGroup - 1)) == 0) same[tid / kScanGroup] = ((ok >> tid) & kAll) == kAll ? alone : -1;
        }
        __syncthreads();
        if (t0 + kScanChunk < a.n_t) load_chunk(t0 + kScanChunk);
        // ---- the chain
        // the state of sequence s0 into the register (the one held goes to dst first)
        auto take = [&](int s0) {
            if (cur >= 0 && valid) ds[cur * seq + mine] = state;
            state = valid ? from[s0 * seq + mine] : 0.0f;
            cur = s0;
        };
        for (int g = 0; g < nt; g += kScanGroup) {
            const int sg = __builtin_amdgcn_readfirstlane(same[g / kScanGroup]);
            if (sg >= 0) {
                if (sg != cur) take(sg);
                float dA[kScanGroup], dBx[kScanGroup], cc[kScanGroup];
#pragma unroll
                for (int j = 0; j < kScanGroup; j++) {
                    const float2 v = dx[g + j][rl];
                    const float2 w = bc[g + j][n];
                    dA[j] = expf(v.x * An);
                    dBx[j] = w.x * v.y;
                    cc[j] = w.y;
                }
                float mine_y = 0.0f;
#pragma unroll
                for (int j = 0; j < kScanGroup; j++) {
                    state = __builtin_fmaf(state, dA[j], dBx[j]);
                    const float y = row16_sum(state * cc[j]);
                    mine_y = n == j ? y : mine_y;
                }
                if (n < kScanGroup) ys[g + n][rl] = mine_y;
                continue;
            }
            for (int tt = g; tt < min(g + kScanGroup, nt); tt++) {
                const int s0 = __builtin_amdgcn_readfirstlane(sq0[tt]);
                if (s0 < 0) continue;
                if (s0 != cur) take(s0);
                const float2 v = dx[tt][rl];
                const float2 w = bc[tt][n];
                state = __builtin_fmaf(state, expf(v.x * An), w.x * v.y);
                const float y = row16_sum(state * w.y);
                if (n == 0) ys[tt][rl] = y;
                if (MULTI) {
                    const int32_t * sq = sq_row(a.sq, a.sq_nb1, t0 + tt);
                    for (int i3 = 1; i3 < a.n_kv; i3++) {
                        const int to = sq[i3];
                        if (to < 0 || to >= a.n_kv) break;
                        if (valid) ds[to * seq + mine] = state;
                    }
                }
            }
        }
        __syncthreads();
        // ---- y of this chunk; the next chunk's staging overwrites dx / bc / sq0 only after this barrier,
        // and its chain writes ys only after the barrier that follows the staging
#pragma unroll
        for (int k = 0; k < kScanChunk * kScanRows / (kScanRows * 16); k++) {
            const int idx = tid + k * kScanRows * 16;
            const int tt = idx >> 4, e = idx & 15;
            if (tt < nt && row0 + e < a.d_inner && sq0[tt] >= 0) a.dst[(size_t) (t0 + tt) * a.d_inner + row0 + e] = ys[tt][e];
        }
        __syncthreads();
    }
    if (cur >= 0 && valid) ds[cur * seq + mine] = state;
}

// ---- ssm_scan, any d_state: one lane per row, the states in dst, the reference's loop (correctness only) ----
constexpr int kScanGenericBlock = 64;

__global__ __launch_bounds__(kScanGenericBlock) void k_ssm_scan_generic(ssm_scan_args a) {
    const int r = blockIdx.x * kScanGenericBlock + threadIdx.x;
    if (r >= a.d_inner) return;
    const int nc = a.d_state;
    float * ds = a.dst + (size_t) a.d_inner * a.n_t;
    const size_t seq = (size_t) nc * a.d_inner;
    for (int i3 = 0; i3 < a.n_kv; i3++) {
        for (int i0 = 0; i0 < nc; i0++) ds[i3 * seq + (size_t) r * nc + i0] = a.s[i3 * seq + (size_t) r * nc + i0];
    }
    const float * A = (const float *) (a.A + (size_t) r * a.A_nb1);
    for (int t = 0; t < a.n_t; t++) {
        const int32_t * sq = sq_row(a.sq, a.sq_nb1, t);
        const int s0 = sq[0];
        if (s0 < 0 || s0 >= a.n_kv) continue;
        const float dtsp = softplus_ref(*(const float *) (a.dt + (size_t) t * a.dt_nb1 + (size_t) r * sizeof(float)));
        const float xdt = a.x[(size_t) t * a.d_inner + r] * dtsp;
        const float * B = (const float *) (a.B + (size_t) t * a.B_nb1);
        const float * C = (const float *) (a.C + (size_t) t * a.C_nb1);
        float * st = ds + s0 * seq + (size_t) r * nc;
        float sum = 0.0f;
        for (int i0 = 0; i0 < nc; i0++) {
            const float state = __builtin_fmaf(st[i0], expf(dtsp * A[i0]), B[i0] * xdt);
            sum += state * C[i0];
            st[i0] = state;
        }
        a.dst[(size_t) t * a.d_inner + r] = sum;
        for (int i3 = 1; i3 < a.n_kv; i3++) {
            const int to = sq[i3];
            if (to < 0 || to >= a.n_kv) break;
            if (to == s0) continue;
            float * st1 = ds + to * seq + (size_t) r * nc;
            for (int i0 = 0; i0 < nc; i0++) st1[i0] = st[i0];
        }
    }
}

template <int NC>
void launch_conv(const ssm_conv_args & a, hipStream_t st) {
    hipLaunchKernelGGL(k_ssm_conv<NC>, dim3((unsigned) ((a.d_inner + kConvBlock - 1) / kConvBlock)), dim3(kConvBlock), 0, st, a);
}

} // namespace

bool mi_ssm_conv_width_ok(int64_t d_conv) { return d_conv >= 2 && d_conv <= 8; }

void mi_op_ssm_conv(const mi_tensor_desc & d, const mi_tensor_desc & s, const mi_tensor_desc & x, const mi_tensor_desc & c,
                    const mi_tensor_desc & sq, hipStream_t st) {
    const int64_t d_conv = c.ne[0], d_inner = c.ne[1], n_t = x.ne[1], n_kv = s.ne[2];
    // refused by supports_op
    if (!mi_ssm_conv_width_ok(d_conv) || s.ne[0] != d_conv - 1 || s.ne[1] != d_inner || x.ne[0] != d_inner || sq.ne[0] != n_kv ||
        sq.ne[1] != n_t || d.ne[0] != d_inner * n_t + d_conv * d_inner * n_kv || d_inner > INT_MAX || n_t > INT_MAX || n_kv > INT_MAX)
        abort();
    if (d_inner <= 0 || n_kv <= 0) return;
    ssm_conv_args a;
    a.s = s.data;
    a.x = x.data;
    a.c = (const float *) c.data;
    a.sq = sq.data;
    a.dst = (float *) d.data;
    a.d_inner = (int) d_inner;
    a.n_t = (int) n_t;
    a.n_kv = (int) n_kv;
    a.s_nb2 = s.nb[2];
    a.x_nb1 = x.nb[1];
    a.sq_nb1 = sq.nb[1];
    switch (d_conv) {
        case 2: launch_conv<2>(a, st); break;
        case 3: launch_conv<3>(a, st); break;
        case 4: launch_conv<4>(a, st); break;
        case 5: launch_conv<5>(a, st); break;
        case 6: launch_conv<6>(a, st); break;
        case 7: launch_conv<7>(a, st); break;
        default: launch_conv<8>(a, st); break;
    }
}

void mi_op_ssm_scan(const mi_tensor_desc & d, const mi_tensor_desc & s, const mi_tensor_desc & x, const mi_tensor_desc & dt,
                    const mi_tensor_desc & A, const mi_tensor_desc & B, const mi_tensor_desc & C, const mi_tensor_desc & sq,
                    hipStream_t st) {
    const int64_t d_state = s.ne[0], d_inner = s.ne[1], n_kv = s.ne[2], n_t = x.ne[1];
    // refused by supports_op
    if (d_state < 1 || x.ne[0] != d_inner || dt.ne[0] != d_inner || dt.ne[1] != n_t || A.ne[0] != d_state || A.ne[1] != d_inner ||
        B.ne[0] != d_state || B.ne[1] != n_t || C.ne[0] != d_state || C.ne[1] != n_t || sq.ne[0] != n_kv || sq.ne[1] != n_t ||
        d.ne[0] != d_inner * n_t + d_state * d_inner * n_kv || d_state > INT_MAX || d_inner > INT_MAX || n_t > INT_MAX ||
        n_kv > INT_MAX)
        abort();
    if (d_inner <= 0 || n_kv <= 0) return;
    ssm_scan_args a;
    a.s = (const float *) s.data;
    a.x = (const float *) x.data;
    a.dt = dt.data;
    a.A = A.data;
    a.B = B.data;
    a.C = C.data;
    a.sq = sq.data;
    a.dst = (float *) d.data;
    a.d_state = (int) d_state;
    a.d_inner = (int) d_inner;
    a.n_t = (int) n_t;
    a.n_kv = (int) n_kv;
    a.dt_nb1 = dt.nb[1];
    a.A_nb1 = A.nb[1];
    a.B_nb1 = B.nb[1];
    a.C_nb1 = C.nb[1];
    a.sq_nb1 = sq.nb[1];
    if (d_state == 16) {
        const dim3 grid((unsigned) ((d_inner + kScanRows - 1) / kScanRows)), block(kScanRows * 16);
        if (n_kv > 1) hipLaunchKernelGGL(k_ssm_scan16<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_ssm_scan16<false>, grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL(k_ssm_scan_generic, dim3((unsigned) ((d_inner + kScanGenericBlock - 1) / kScanGenericBlock)),
                           dim3(kScanGenericBlock), 0, st, a);
    }
}
