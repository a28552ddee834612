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
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

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
    {"mmq_variant", &mi_tuning::mmq_variant, INT_MIN, kAny, nullptr},
    {"attn_variant", &mi_tuning::attn_variant, INT_MIN, kAny, nullptr},
    {"mmv_order", &mi_tuning::mmv_order, -1, 1, nullptr},
    {"f16_waves", &mi_tuning::f16_waves, 0, kAny, nullptr},
    {"f16_rgs", &mi_tuning::f16_rgs, 0, 8, nullptr},
    {"f16_ps_waves", &mi_tuning::f16_ps_waves, 0, 8, [](int v) { return v == 0 || v == 2 || v == 4 || v == 8; }},
    {"xfirst", &mi_tuning::xfirst, -1, 1, nullptr},
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

bool mi_tuning_set(const char * name, int value) { return knob_set(g_mi_tuning, name, value); }

// per-format launchers (mmv_fused_q4k.hip, _q5k, _q6k, _q40, _q80, _q41, _q50, _q51: one translation unit each)
void mi_mmv_launch_q4k(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q5k(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q40(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q80(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q6k(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q41(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q50(const mi_mmv_group & g, int variant, hipStream_t s);
void mi_mmv_launch_q51(const mi_mmv_group & g, int variant, hipStream_t s);

// LDS of the quantized activations: qs [NC][K] int8 | d [NC][K/QKA] f32 | s32 [NC][K/32] int16
// (lds_bytes in mmv_fused_impl.h)
size_t mi_mmv_fused_lds_bytes(int type, int64_t K, int64_t ncols) {
    const int nc = ncols <= 2 ? (int) ncols : (ncols <= 4 ? 4 : 8);
    const int64_t qka = (type == 12 || type == 13 || type == 14) ? 256 : 32;
    return (size_t) nc * (K + (K / qka) * 4 + (K / 32) * 2);
}

bool mi_mmv_fused_supported(int type, int64_t K, int64_t ncols) {
    if (type != 12 && type != 13 && type != 14 && type != 2 && type != 8 && type != 3 && type != 6 && type != 7) return false;
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
    // variant 0 = per-type default, from interleaved A/B runs on MI355X (tools/mmv_tune.py):
    // prefetch depth 2 for Q4_K / Q8_0 / Q4_0 (Q4_0 in block pairs: 4096 x 11008 5.34 -> 5.58
    // TB/s), depth 1 for Q5_K (fewer VGPRs, more waves)
    // (Nontemporal weight loads -- the guide's nt-weights -- measured 30-37 % SLOWER on every
    // shape, profiles/r04g_nt_ab.txt: removed.) Round-4 defaults from two interleaved sweeps on two
    // boxes (profiles/r04p_gemv_sweep.txt, r04r_gemv_sweep.txt): Q4_K depth 3 (4096^2 +2..4 %,
    // 4096 x 11008 +2..4 %), Q5_K depth 2 (+2 %), Q4_0 pairs depth 3 (+1..4 %), Q8_0 depth 1 (+1 %)
    int variant = g_mi_tuning.mmv_variant;
    // (Q4_1 / Q5_0 / Q5_1: depth 2 like the other 5- and 6-dword items, not tuned: DESIGN section 14)
    if (variant == 0)
        variant = g.type == 12 ? 31 : g.type == 13 || g.type == 14 || g.type == 3 || g.type == 6 || g.type == 7 ? 21 : g.type == 2 ? 32 : 11;
    switch (g.type) {
        case 12: mi_mmv_launch_q4k(g, variant, s); break;
        case 13: mi_mmv_launch_q5k(g, variant, s); break;
        case 14: mi_mmv_launch_q6k(g, variant, s); break;
        case 3: mi_mmv_launch_q41(g, variant, s); break;
        case 6: mi_mmv_launch_q50(g, variant, s); break;
        case 7: mi_mmv_launch_q51(g, variant, s); break;
        case 2: mi_mmv_launch_q40(g, variant, s); break;
        case 8: mi_mmv_launch_q80(g, variant, s); break;
        default: break;
    }
}
