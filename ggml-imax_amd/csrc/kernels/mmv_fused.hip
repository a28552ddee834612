// mmv_fused.hip -- decode-regime GGML_OP_MUL_MAT with the activation quantizer fused in, and
// several independent mul_mat nodes of one graph served by a single streaming launch.
//
// Structure (HBM-bound weight stream; MI355X_MICROARCH.md: 8 TB/s, ~6.3 TB/s achievable):
//   * grid = ~4 workgroups per CU (all resident); each workgroup owns a contiguous row range of
//     ONE group member (blockIdx.x -> member, row range), so the activation quantization is paid
//     once per workgroup, not per row;
//   * prologue: issue the weight loads of the first rows (global loads straight to VGPRs), then
//     quantize the member's NC f32 activation columns into LDS with the reference's exact
//     rounding (Q8_K for Q4_K/Q5_K, AVX2-path Q8_0 for Q4_0/Q8_0), barrier;
//   * stream: wave w walks rows w, w+4, ... keeping PD rows of loads in flight in a register ring
//     ahead of the row being computed; v_dot4_i32_i8 against the LDS activations; DPP wave
//     reduction; one store per row.
// A lane's K-items are the same for every row: item = lane + 64*i. Items:
//   Q4_K / Q5_K: (superblock s, 64-element group j): 16 B header + 32 B nibbles (+32 B qh),
//                aligned dwordx4 loads; a K=4096 row is one item per lane.
//   Q4_0 / Q8_0: one 32-element block (18 / 34 B, only 2-byte aligned): aligned dword loads
//                re-aligned with v_alignbyte; a K=4096 row is two items per lane.
//
// Numerics: bit-exact activation quants, exact integer sums per item, f32 combination, i.e.
// ggml_vec_dot_q4_K_q8_K (src/ggml-quants.c:7007-7502), ggml_vec_dot_q5_K_q8_K (:7833-8378),
// ggml_vec_dot_q4_0_q8_0 (:3469-3874), ggml_vec_dot_q8_0_q8_0 (:4819+) up to summation order.


#include "mi355x_common.h"
#include "mi355x_kernels.h"


#include <ctype.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <unordered_map>

// The one list of knobs: set_tuning(name, v) and GGML_MI355X_<NAME>=v (read once at start-up) both go
// through mi_tuning_set, so both accept lo <= v <= hi (and ok(v) where a knob takes only some values).
namespace {
constexpr int kAny = INT_MAX;
struct knob {
    const char * name;
    int mi_tuning::*field;
    int lo, hi;
    bool (*ok)(int);
};
const knob kKnobs[] = {
    {"mmv_blocks", &mi_tuning::mmv_blocks, 0, kAny, nullptr},
    {"mmv_variant", &mi_tuning::mmv_variant, INT_MIN, kAny, nullptr},
    {"f16_variant", &mi_tuning::f16_variant, INT_MIN, kAny, nullptr},
    {"f16_threads", &mi_tuning::f16_threads, 0, 256, [](int v) { return v == 0 || v == 64 || v == 128 || v == 256; }},
    {"mmq_variant", &mi_tuning::mmq_variant, 0, kMmqVariantMask, [](int v) { return (v & ~kMmqVariantMask) == 0; }},
    {"attn_variant", &mi_tuning::attn_variant, INT_MIN, kAny, nullptr},
    {"mmv_order", &mi_tuning::mmv_order, -1, 1, nullptr},
    {"f16_waves", &mi_tuning::f16_waves, 0, kAny, nullptr},
    {"f16_rgs", &mi_tuning::f16_rgs, 0, 8, nullptr},
    {"f16_ps_waves", &mi_tuning::f16_ps_waves, 0, 8, [](int v) { return v == 0 || v == 2 || v == 4 || v == 8; }},
    {"f16_norm_waves", &mi_tuning::f16_norm_waves, 0, 8, nullptr},
    {"planes", &mi_tuning::planes, 0, 1, nullptr},
    {"f16_nc", &mi_tuning::f16_nc, 0, 88, [](int v) { return v % 10 <= 8; }},
    {"f16_bn", &mi_tuning::f16_bn, 0, 15, [](int v) { return v % 10 <= 5; }},
    {"q40r", &mi_tuning::q40r, 0, 1, nullptr},
    {"q80r", &mi_tuning::q80r, 0, 1, nullptr},
    {"mmv_pro4", &mi_tuning::mmv_pro4, 0, 1, nullptr},
    {"f16_mt", &mi_tuning::f16_mt, 0, 1, nullptr},
    {"mmqt_short", &mi_tuning::mmqt_short, 0, kAny, nullptr},
    {"mmid_group", &mi_tuning::mmid_group, 0, 8, [](int v) { return v == 0 || v == 1 || v == 4 || v == 8; }},
    {"mmid_stream", &mi_tuning::mmid_stream, 0, 8, nullptr},
    {"fuse_router", &mi_tuning::fuse_router, 0, 1, nullptr},
    {"ord_prefill_cols", &mi_tuning::ord_prefill_cols, 0, kAny, nullptr},
    {"tree_prefill_cols", &mi_tuning::tree_prefill_cols, 0, kAny, nullptr},
};

bool knob_set(mi_tuning & t, const char * name, int value) {
    for (const knob & k : kKnobs) {
        if (strcmp(name, k.name) != 0) continue;
        if (value < k.lo || value > k.hi || (k.ok && !k.ok(value))) return false;
        t.*k.field = value;
        return true;
    }
    return false;
}

mi_tuning tuning_from_env() {
    mi_tuning t;
    for (const knob & k : kKnobs) {
        std::string env = "GGML_MI355X_";
        for (const char * c = k.name; *c; c++) env += (char) toupper((unsigned char) *c);
        const char * v = getenv(env.c_str());
        if (v && !knob_set(t, k.name, atoi(v))) fprintf(stderr, "%s=%s: value not accepted, keeping the default %d\n", env.c_str(), v, t.*k.field);
    }
    return t;
}
}  // namespace

mi_tuning g_mi_tuning = tuning_from_env();
thread_local int tl_mi_graph_order = 0;
const char * g_mi_last_route = "";

void mi_route_fmt(uint32_t key, const char * fmt, ...) {
    static std::mutex mu;
    static std::unordered_map<uint32_t, std::string> names;  // (node-based: a stored string never moves)
    std::lock_guard<std::mutex> lock(mu);
    auto it = names.find(key);
    if (it == names.end()) {
        char buf[128];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        it = names.emplace(key, buf).first;
    }
    g_mi_last_route = it->second.c_str();
}

bool mi_tuning_set(const char * name, int value) { return knob_set(g_mi_tuning, name, value); }


// LDS of the quantized activations: qs [NC][K] int8 | d [NC][K/QKA] f32 | s32 [NC][K/32] int16
// (lds_bytes in mmv_fused_impl.h)
size_t mi_mmv_fused_lds_bytes(int type, int64_t K, int64_t ncols) {
    const int nc = ncols <= 2 ? (int) ncols : (ncols <= 4 ? 4 : 8);
    const int64_t qka = mi_act_block(mi_type(type).act);
    return (size_t) nc * (K + (K / qka) * 4 + (K / 32) * 2);
}

bool mi_mmv_fused_supported(int type, int64_t K, int64_t ncols) {
    if (!mi_type(type).mmv_variant) return false;
    if (ncols < 1 || ncols > 8 || K % 256 != 0) return false;
    // more than 4 columns whose activations do not fit run as two launches of <= 4 columns
    return mi_mmv_fused_lds_bytes(type, K, ncols < 4 ? ncols : 4) <= 64 * 1024;  // + <= 36 KB of order scratch
}



static void mi_mul_mat_q_fused_launch(mi_mmv_group & g, hipStream_t s);

void mi_mul_mat_q_fused(mi_mmv_group & g, hipStream_t s) {
    if (g.ncols > 4 && mi_mmv_fused_lds_bytes(g.type, g.K, g.ncols) > 64 * 1024) {
        for (int c0 = 0; c0 < g.ncols; c0 += 4) {
            mi_mmv_group h = g;
            h.ncols = g.ncols - c0 < 4 ? g.ncols - c0 : 4;
            for (int m = 0; m < g.n; m++) {
                h.m[m].X = g.m[m].X + (size_t) c0 * g.xcol;
                h.m[m].dst = (float *) ((char *) g.m[m].dst + (size_t) c0 * g.ycol);
            }
            if (h.epi.resid) h.epi.resid += (size_t) c0 * h.epi.resid_nb1;
            for (auto & cp : h.epi.copy)
                if (cp.ptr) cp.ptr += (size_t) c0 * cp.col_stride;
            mi_mul_mat_q_fused_launch(h, s);
        }
        return;
    }
    mi_mul_mat_q_fused_launch(g, s);
}

static void mi_mul_mat_q_fused_launch(mi_mmv_group & g, hipStream_t s) {
    // variant 0 = the per-type default (the table in mi355x_types.h, with the measurements behind it)
    int variant = g_mi_tuning.mmv_variant;
    if (variant == 0) variant = mi_type(g.type).mmv_variant;
    mi_dispatch_type(g.type, [&](auto t) {
        constexpr int T = decltype(t)::value;
        if constexpr (mi_type(T).mmv_variant != 0) mi_mmv_launch<T>(g, variant, s);
        else MI_ASSERT(!"no streaming GEMV for this weight type");
    });
}
