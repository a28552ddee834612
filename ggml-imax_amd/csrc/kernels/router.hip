// router.hip -- the ops of a mixture-of-experts router on gfx950, each the reference CPU's bits:
//   sum_rows   src/ggml.c:10159-10192 (ggml_vec_sum_f32, :2080: a sequential double sum rounded once)
//   argsort    src/ggml.c:15064-15105 (an in-place exchange sort with strict comparisons)
//   the chain  soft_max -> argsort DESC -> first k -> get_rows(probs) -> sum_rows -> div in one launch
//
// ARGSORT. Pass j of the reference loop carries idx[j] over the positions k > j and swaps wherever
// position k's value is strictly better. After the pass idx[j] is the first-occurring best of [j, n),
// every position p > j whose value was strictly better than all of [j, p) holds the previous record
// (the first-occurring best of [j, p)), and everything else is where it was. So a pass is an
// exclusive prefix "arg-best, earliest on ties" scan: the workgroup kernel (rows of 65 .. 1024) runs
// that scan, log2 steps per pass; a single wave (rows up to 64, and the fused router) instead steps
// through the pass's swaps with ballots, which are few. A row without equal values has one answer
// (out[number of strictly better elements] = i) and needs no pass. ASC sorts the negated values
// (x -> -x reverses every strict comparison and keeps +0 == -0). Positions past the row hold -inf:
// they lie to the right of every real position and only a strictly better value displaces a record,
// so they never enter a result. NaN is not handled.

#include "mi355x_common.h"
#include "mi355x_kernels.h"

#include "cpu_order.h"

namespace {

__device__ __forceinline__ size_t row_off(const mi_tensor_desc & t, int64_t r) {
    const int64_t i1 = r % t.ne[1];
    r /= t.ne[1];
    return (size_t) i1 * t.nb[1] + (size_t) (r % t.ne[2]) * t.nb[2] + (size_t) (r / t.ne[2]) * t.nb[3];
}

// ---- sum_rows: one wave per row -------------------------------------------------------------------
// The certification of cpu_order.h without the division: a parallel double sum S is within
// B = 4 n 2^-53 sum|x| of the sequential one, so when S - B and S + B round to the same float that
// float is the CPU's; otherwise lane 0 replays the chain.
constexpr int kSumRowsWaves = 4;

__global__ __launch_bounds__(64 * kSumRowsWaves) void k_sum_rows(mi_tensor_desc d, mi_tensor_desc a, int64_t nrows) {
    const int64_t row = (int64_t) blockIdx.x * kSumRowsWaves + (threadIdx.x >> 6);
    if (row >= nrows) return;  // wave-uniform, before any cross-lane op
    const int lane = threadIdx.x & 63;
    const char * x = a.data + row_off(a, row);
    float * y = (float *) (d.data + row_off(d, row));
    const int64_t n = a.ne[0];
    bool chain = n <= 8;
    if (!chain) {
        double s = 0.0, m = 0.0;
        for (int64_t i = lane; i < n; i += 64) {
            const double t = (double) *(const float *) (x + i * sizeof(float));
            s += t;
            m += fabs(t);
        }
        s = mi_wave_sum_u_f64(s);
        m = mi_wave_sum_u_f64(m);
        const double B = 4.0 * (double) n * m * 0x1p-53 + 0x1p-1074;
        const float lo = (float) (s - B);
        const float hi = (float) (s + B);
        if (lo == hi) {
            if (lane == 0) *y = lo == 0.0f ? 0.0f : lo;  // the CPU's chain starts at +0.0
        } else {
            chain = true;
        }
    }
    if (chain && lane == 0) {
        double q = 0.0;
        for (int64_t i = 0; i < n; i++) q += (double) *(const float *) (x + i * sizeof(float));
        *y = (float) q;
    }
}

// ---- argsort ----------------------------------------------------------------------------------------

// inclusive scan over the wave's lanes of (best value, its first position) restricted to positions
// >= j: lane l ends with the first-occurring best of [max(j, pos - l), pos]
__device__ __forceinline__ void wave_scan_best(int j, int pos, int lane, float & bv, int & bp) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float tv = __shfl_up(bv, off, 64);
        const int tp = __shfl_up(bp, off, 64);
        if (lane >= off && pos - off >= j && !(bv > tv)) {
            bv = tv;
            bp = tp;
        }
    }
}

__device__ __forceinline__ float wave_read(float v, int l) {  // lane l's value, l wave-uniform (v_readlane)
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// one pass of the exchange sort on a row held one position per lane (w: the value at the position,
// id: its index; lanes past the row hold -inf): the reference's inner loop itself, stepping from one
// swap to the next. The record carried at position j moves only where a later position is strictly
// better -- found with a ballot -- and that position receives the record it displaces. At most as
// many steps as the row has distinct values. The whole wave calls it; every branch is wave-uniform.
__device__ __forceinline__ void wave_pass(int j, int lane, float & w, int & id) {
    float rv = wave_read(w, j);
    int rid = __builtin_amdgcn_readlane(id, j);
    int cur = j;
    for (;;) {
        const unsigned long long later = cur >= 63 ? 0ull : ~0ull << (cur + 1);
        const unsigned long long b = __ballot(w > rv);
        // (the ballot is the same in every lane: read into scalar registers, so the loop stays scalar)
        const unsigned long long m = (((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (b >> 32)) << 32) |
                                      (unsigned) __builtin_amdgcn_readfirstlane((int) b)) & later;
        if (m == 0) break;
        const int p = __builtin_ctzll(m);
        const float nv = wave_read(w, p);
        const int nid = __builtin_amdgcn_readlane(id, p);
        if (lane == p) {
            w = rv;
            id = rid;
        }
        rv = nv;
        rid = nid;
        cur = p;
    }
    if (lane == j) {
        w = rv;
        id = rid;
    }
}

// a row of at most 64 values in a wave, lane l = element l: the lane's position in the sorted row
// (strictly better elements), *ties = some value occurs twice (wave-uniform)
__device__ __forceinline__ int wave_rank(float w, int n, int lane, bool * ties) {
    int gt = 0, eq = 0;
    for (int l = 0; l < n; l++) {
        const float t = wave_read(w, l);
        gt += t > w;
        eq += t == w;
    }
    *ties = __any(lane < n && eq > 1);
    return gt;
}

// sorts the wave's row: on return lane p < n holds the value and index of sorted position p, for
// p < n_sorted (the reference's first n_sorted passes; n_sorted = n: the whole permutation)
__device__ __forceinline__ void wave_argsort(float & w, int & id, int n, int n_sorted, int lane) {
    bool ties;
    const int rank = wave_rank(w, n, lane, &ties);
    if (!ties) {
        // push each element to the lane of its rank (a permutation; lanes past the row to themselves)
        const int to = (lane < n ? rank : lane) << 2;
        id = __builtin_amdgcn_ds_permute(to, lane);
        w = __int_as_float(__builtin_amdgcn_ds_permute(to, __float_as_int(w)));
        return;
    }
    const int passes = n_sorted < n - 1 ? n_sorted : n - 1;
    for (int j = 0; j < passes; j++) wave_pass(j, lane, w, id);
}

constexpr int kArgsortWaves = 4;

// rows of at most 64 elements: one wave per row
__global__ __launch_bounds__(64 * kArgsortWaves) void k_argsort_wave(mi_tensor_desc d, mi_tensor_desc a, int64_t nrows, int descending) {
    const int64_t row = (int64_t) blockIdx.x * kArgsortWaves + (threadIdx.x >> 6);
    if (row >= nrows) return;  // wave-uniform, before any cross-lane op
    const int lane = threadIdx.x & 63;
    const int n = (int) a.ne[0];
    const float * x = (const float *) (a.data + (size_t) row * a.nb[1]);
    int32_t * y = (int32_t *) (d.data + (size_t) row * d.nb[1]);
    float w = -INFINITY;
    if (lane < n) w = descending ? x[lane] : -x[lane];
    int id = lane;
    wave_argsort(w, id, n, n, lane);
    if (lane < n) y[lane] = id;
}

// rows of 65 .. 1024 elements: one workgroup per row, one position per thread
__global__ __launch_bounds__(kMiArgsortMaxRow) void k_argsort_block(mi_tensor_desc d, mi_tensor_desc a, int descending) {
    __shared__ float sval[kMiArgsortMaxRow];
    __shared__ int sidx[kMiArgsortMaxRow];
    __shared__ float swv[kMiArgsortMaxRow / 64];
    __shared__ int swp[kMiArgsortMaxRow / 64];
    const int p = threadIdx.x, lane = p & 63, wave = p >> 6, nw = (int) (blockDim.x >> 6);
    const int n = (int) a.ne[0];
    const float * x = (const float *) (a.data + (size_t) blockIdx.x * a.nb[1]);
    int32_t * y = (int32_t *) (d.data + (size_t) blockIdx.x * d.nb[1]);
    float w = -INFINITY;
    if (p < n) w = descending ? x[p] : -x[p];
    sval[p] = w;
    sidx[p] = p;
    __syncthreads();
    int gt = 0, eq = 0;
    if (p < n) {
        for (int l = 0; l < n; l++) {
            const float t = sval[l];
            gt += t > w;
            eq += t == w;
        }
    }
    if (!__syncthreads_or(eq > 1)) {  // uniform over the workgroup
        if (p < n) y[gt] = p;
        return;
    }
    int id = p;
    for (int j = 0; j < n - 1; j++) {
        float bv = w;
        int bp = p;
        wave_scan_best(j, p, lane, bv, bp);
        if (lane == 63) {
            swv[wave] = bv;
            swp[wave] = bp;
        }
        const float ev = __shfl_up(bv, 1, 64);
        const int ep = __shfl_up(bp, 1, 64);
        __syncthreads();
        int nid = id;
        float nwv = w;
        if (p >= j && p < n) {
            // the first-occurring best of the waves before this one (from j's wave on), then of
            // [j, p) -- or, for position j itself, of the whole of [j, n)
            const int w0 = j >> 6;
            bool have = false;
            float av = 0.0f;
            int ap = 0;
            const int w1 = p == j ? nw : wave;
            for (int v = w0; v < w1; v++) {
                if (!have || swv[v] > av) {
                    av = swv[v];
                    ap = swp[v];
                    have = true;
                }
            }
            if (p > j && lane > 0 && p - 1 >= j && (!have || ev > av)) {
                av = ev;
                ap = ep;
                have = true;
            }
            if (p == j || (have && w > av)) {
                nid = sidx[ap];
                nwv = av;
            }
        }
        __syncthreads();
        id = nid;
        w = nwv;
        sidx[p] = id;
    }
    if (p < n) y[p] = id;
}

// ---- the router chain: one wave per token ---------------------------------------------------------------
constexpr int kRouterWaves = 4;

__global__ __launch_bounds__(64 * kRouterWaves) void k_router(mi_router_desc r, const uint16_t * exp_table) {
    const int64_t t = (int64_t) blockIdx.x * kRouterWaves + (threadIdx.x >> 6);
    if (t >= r.T) return;  // wave-uniform, before any cross-lane op
    const int lane = threadIdx.x & 63;
    const int n = r.n_expert, k = r.k;
    // soft_max with scale 1 and no mask, as k_soft_max (ops.hip): fp16 exp table, exact double sum
    const float x = lane < n ? r.logits[t * n + lane] : -INFINITY;
    const float mx = mi_wave_max(x);
    const float v = x == -INFINITY ? 0.0f : mi_h2f(exp_table[mi_f2h(sub_rn(x, mx))]);
    const double sum = mi_wave_sum_u_f64((double) v);
    const float inv = (float) (1.0 / sum);
    const float prob = mul_rn(v, inv);
    if (lane < n) r.probs[t * n + lane] = prob;
    // argsort DESC: sorted position p in lane p
    float w = lane < n ? prob : -INFINITY;
    int id = lane;
    wave_argsort(w, id, n, r.n_sorted, lane);
    if (lane < r.n_sorted) r.sorted[t * n + lane] = id;
    // get_rows: the selected probabilities; sum_rows: their sequential double sum; div
    if (lane < k) r.weights[t * k + lane] = w;
    if (r.sums) {
        double q = 0.0;
        for (int j = 0; j < k; j++) q += (double) wave_read(w, j);
        const float s = (float) q;
        if (lane == 0) r.sums[t] = s;
        if (lane < k) r.normed[t * k + lane] = w / s;
    }
}

} // namespace

void mi_op_sum_rows(const mi_tensor_desc & d, const mi_tensor_desc & a, hipStream_t s) {
    const int64_t rows = a.ne[1] * a.ne[2] * a.ne[3];
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_sum_rows, dim3((unsigned) ((rows + kSumRowsWaves - 1) / kSumRowsWaves)), dim3(64 * kSumRowsWaves), 0, s, d, a, rows);
}

void mi_op_argsort(const mi_tensor_desc & d, const mi_tensor_desc & a, bool descending, hipStream_t s) {
    const int64_t rows = a.ne[1] * a.ne[2] * a.ne[3];
    const int64_t n = a.ne[0];
    if (n > kMiArgsortMaxRow) abort();  // refused by supports_op
    if (rows <= 0 || n <= 0) return;
    if (n <= 64) {
        hipLaunchKernelGGL(k_argsort_wave, dim3((unsigned) ((rows + kArgsortWaves - 1) / kArgsortWaves)), dim3(64 * kArgsortWaves), 0, s, d, a,
                           rows, descending ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_argsort_block, dim3((unsigned) rows), dim3((unsigned) ((n + 63) / 64 * 64)), 0, s, d, a, descending ? 1 : 0);
    }
}

void mi_router_fused(const mi_router_desc & r, const uint16_t * exp_table, hipStream_t s) {
    if (r.n_expert > kMiRouterMaxExperts || r.k > r.n_expert) abort();  // the fusion pass checks both
    if (r.T <= 0) return;
    hipLaunchKernelGGL(k_router, dim3((unsigned) ((r.T + kRouterWaves - 1) / kRouterWaves)), dim3(64 * kRouterWaves), 0, s, r, exp_table);
}
