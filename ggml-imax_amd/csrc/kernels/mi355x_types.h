// mi355x_types.h -- the one table of weight types: what the kernels, their launchers and the backend
// know about a ggml_type (block geometry, the activation quantization it dots with, the routes
// that read it), and the dispatch from a run-time type to a compile-time one.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define MI_ASSERT(x)                                                                                    \
    do {                                                                                                \
        if (!(x)) {                                                                                     \
            fflush(stdout);                                                                             \
            fprintf(stderr, "ggml-mi355x: assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #x);  \
            abort();                                                                                    \
        }                                                                                               \
    } while (0)

// the ggml_type values the kernels use (the kernel directory does not see the ggml ABI header: the
// backend static_asserts each against GGML_TYPE_*). Kernel templates take them as plain ints.
constexpr int MI_TYPE_F32 = 0, MI_TYPE_F16 = 1, MI_TYPE_Q4_0 = 2, MI_TYPE_Q4_1 = 3, MI_TYPE_Q5_0 = 6, MI_TYPE_Q5_1 = 7,
              MI_TYPE_Q8_0 = 8, MI_TYPE_Q8_1 = 9, MI_TYPE_Q2_K = 10, MI_TYPE_Q3_K = 11, MI_TYPE_Q4_K = 12, MI_TYPE_Q5_K = 13, MI_TYPE_Q6_K = 14, MI_TYPE_Q8_K = 15,
              MI_TYPE_IQ4_NL = 20, MI_TYPE_IQ4_XS = 23, MI_TYPE_I32 = 26, MI_TYPE_BF16 = 30;

// How the activation columns of a mul_mat are quantized: the weight type's vec_dot_type in the
// reference (src/ggml.c type_traits). MI_ACT_NONE: F32 weights read src1 as it lies. MI_ACT_F16 /
// MI_ACT_BF16: dense 2-byte elements (ggml_fp32_to_fp16_row / ggml_fp32_to_bf16_row), no blocks.
enum mi_act_quant : int { MI_ACT_NONE, MI_ACT_Q8_0, MI_ACT_Q8_1, MI_ACT_Q8_K, MI_ACT_F16, MI_ACT_BF16 };
constexpr int mi_act_block(mi_act_quant q) { return q == MI_ACT_Q8_K ? 256 : 32; }  // elements per q8 block
constexpr int mi_act_block_bytes(mi_act_quant q) {  // bytes per block of its rows in the reference layout (block_q8_0 / _q8_1 / _q8_K)
    return q == MI_ACT_Q8_K ? 292 : q == MI_ACT_Q8_1 ? 36 : q == MI_ACT_Q8_0 ? 34 : 2;
}
constexpr int mi_act_type(mi_act_quant q) {  // its ggml_type (-1: none)
    return q == MI_ACT_Q8_0 ? MI_TYPE_Q8_0 : q == MI_ACT_Q8_1 ? MI_TYPE_Q8_1 : q == MI_ACT_Q8_K ? MI_TYPE_Q8_K : q == MI_ACT_F16 ? MI_TYPE_F16 : q == MI_ACT_BF16 ? MI_TYPE_BF16 : -1;
}

struct mi_type_info {
    int type;          // ggml_type, -1: not a weight type of this backend
    int blck;          // elements per block: 1, 32 or 256
    int bytes;         // bytes per block
    mi_act_quant act;  // the activations it dots with
    // 32-element blocks (fp16 d [, fp16 m] [, qh[4]], quants): value (q - sub) d [+ m]
    bool has_m;        // fp16 m after d; dots with Q8_1
    bool has_qh;       // a fifth-bit plane qh[4] before the quants
    int sub;           // subtracted from every level
    bool lut;          // the 4-bit levels index the IQ4 codebook (kvalues_iq4nl) instead of counting
    // routes
    int mmv_variant;   // streaming decode GEMV (mi_mul_mat_q_fused): its default mmv_variant, 0: no such kernel
    int mmv_align;     // ... and the weight row alignment it needs (the tensor base: 16)
    bool mmqx;         // exact int8 prefill GEMM (mmq_exact.hip)
    bool planes;       // repacked MFMA planes for long prompts (mmq_planes.hip k_mmqr)
    bool aligned_copy; // 16-byte-aligned decode copy (mmq_planes.hip k_q40_repack / k_q80_repack): as many bytes a row as the blocks
    bool get_rows;     // GET_ROWS reads it (f32 / f16 elements, or the dequantizer of ops.hip)
};

// mmv_variant defaults, from interleaved A/B runs on MI355X (tools/mmv_tune.py):
// prefetch depth 2 for Q4_K / Q8_0 / Q4_0 (Q4_0 in block pairs: 4096 x 11008 5.34 -> 5.58
// TB/s), depth 1 for Q5_K (fewer VGPRs, more waves)
// (Nontemporal weight loads -- the guide's nt-weights -- measured 30-37 % SLOWER on every
// shape, profiles/r04g_nt_ab.txt: removed.) Round-4 defaults from two interleaved sweeps on two
// boxes (profiles/r04p_gemv_sweep.txt, r04r_gemv_sweep.txt): Q4_K depth 3 (4096^2 +2..4 %,
// 4096 x 11008 +2..4 %), Q5_K depth 2 (+2 %), Q4_0 pairs depth 3 (+1..4 %), Q8_0 depth 1 (+1 %)
// (Q4_1 / Q5_0 / Q5_1: depth 2 like the other 5- and 6-dword items, not tuned: DESIGN section 14)
// Q2_K depth 2, Q3_K depth 1 (profiles/q2k_q3k_variant_sweep.txt: no difference beyond the rounds' spread
// at K = 4096; Q3_K 11008 x 4096 -8 % in tree order and -14 % in the reference order at depth 1)
// IQ4_NL / IQ4_XS depth 2 (profiles/iq4_variant_sweep.txt: depths 1 to 3 alike within the rounds' spread)
//
// mmv_align: 16-byte rows, except Q6_K, whose 210-byte blocks its loads re-align themselves (rows
// of an odd superblock count are 2 mod 4: K = 11008 has 9030-byte rows), and likewise Q3_K (110-byte
// blocks: 2) and Q2_K (84-byte blocks: 4). IQ4_XS reads 8-byte words of its 136-byte blocks (rows of an
// odd superblock count are 8 mod 16: K = 11008 has 5848-byte rows): 8.
// planes: Q5_K has the plane format (PFmt) and its repack kernel, but no GEMM that reads them.
constexpr mi_type_info kMiTypes[] = {
    //  type         blck bytes act          has_m  has_qh sub  lut    mmv  align mmqx   planes copy   get_rows
    {MI_TYPE_F32,    1,   4,   MI_ACT_NONE, false, false, 0,   false, 0,   16,   false, false, false, true},
    {MI_TYPE_F16,    1,   2,   MI_ACT_F16,  false, false, 0,   false, 0,   16,   false, false, false, true},
    // (BF16: its own kernels, mm_bf16.hip. Never the F16 GEMMs of mmq.hip or mi_convert_f16: bf16's
    // exponent range does not fit f16. Rows of an odd K are 2-byte aligned: its launchers pick the path.)
    {MI_TYPE_BF16,   1,   2,   MI_ACT_BF16, false, false, 0,   false, 0,   2,    false, false, false, true},
    {MI_TYPE_Q4_0,   32,  18,  MI_ACT_Q8_0, false, false, 8,   false, 32,  16,   true,  false, true,  true},
    {MI_TYPE_Q4_1,   32,  20,  MI_ACT_Q8_1, true,  false, 0,   false, 21,  16,   false, false, false, true},
    {MI_TYPE_Q5_0,   32,  22,  MI_ACT_Q8_0, false, true,  16,  false, 21,  16,   false, false, false, true},
    {MI_TYPE_Q5_1,   32,  24,  MI_ACT_Q8_1, true,  true,  0,   false, 21,  16,   false, false, false, true},
    {MI_TYPE_Q8_0,   32,  34,  MI_ACT_Q8_0, false, false, 0,   false, 11,  16,   true,  false, true,  true},
    {MI_TYPE_Q2_K,   256, 84,  MI_ACT_Q8_K, false, false, 0,   false, 21,  4,    false, false, false, true},
    {MI_TYPE_Q3_K,   256, 110, MI_ACT_Q8_K, false, false, 0,   false, 11,  2,    false, false, false, true},
    {MI_TYPE_Q4_K,   256, 144, MI_ACT_Q8_K, false, false, 0,   false, 31,  16,   true,  true,  false, true},
    {MI_TYPE_Q5_K,   256, 176, MI_ACT_Q8_K, false, false, 0,   false, 21,  16,   true,  false, false, true},
    {MI_TYPE_Q6_K,   256, 210, MI_ACT_Q8_K, false, false, 0,   false, 21,  2,    false, false, false, true},
    {MI_TYPE_IQ4_NL, 32,  18,  MI_ACT_Q8_0, false, false, 0,   true,  21,  16,   false, false, false, true},
    {MI_TYPE_IQ4_XS, 256, 136, MI_ACT_Q8_K, false, false, 0,   true,  21,  8,    false, false, false, true},
};
constexpr mi_type_info kMiNoType = {-1, 1, 0, MI_ACT_NONE, false, false, 0, false, 0, 16, false, false, false, false};

// the row of `type` (kMiNoType: none): a compile-time constant in kernels, a lookup on the host
constexpr mi_type_info mi_type(int type) {
    for (const mi_type_info & t : kMiTypes)
        if (t.type == type) return t;
    return kMiNoType;
}
constexpr bool mi_type_quantized(int type) { return mi_type(type).blck > 1; }

// Calls f(mi_type_c<T>{}) with T == type, for every row of the table, so that a generic lambda gets
// the run-time type as a compile-time constant. A type outside the table stops here (supports_op
// refuses such nodes) instead of running another type's kernel. Launchers that serve a subset of
// the rows test the row's route field with if constexpr and end in MI_ASSERT(!"...") for the rest,
// so only the kernels of that subset are instantiated.
template <int T> struct mi_type_c { static constexpr int value = T; };
template <class F> void mi_dispatch_type(int type, F && f) {
    switch (type) {
        case MI_TYPE_Q4_0: f(mi_type_c<MI_TYPE_Q4_0>{}); break;
        case MI_TYPE_Q8_0: f(mi_type_c<MI_TYPE_Q8_0>{}); break;
        case MI_TYPE_Q4_1: f(mi_type_c<MI_TYPE_Q4_1>{}); break;
        case MI_TYPE_Q5_0: f(mi_type_c<MI_TYPE_Q5_0>{}); break;
        case MI_TYPE_Q5_1: f(mi_type_c<MI_TYPE_Q5_1>{}); break;
        case MI_TYPE_Q2_K: f(mi_type_c<MI_TYPE_Q2_K>{}); break;
        case MI_TYPE_Q3_K: f(mi_type_c<MI_TYPE_Q3_K>{}); break;
        case MI_TYPE_Q4_K: f(mi_type_c<MI_TYPE_Q4_K>{}); break;
        case MI_TYPE_Q5_K: f(mi_type_c<MI_TYPE_Q5_K>{}); break;
        case MI_TYPE_Q6_K: f(mi_type_c<MI_TYPE_Q6_K>{}); break;
        case MI_TYPE_IQ4_NL: f(mi_type_c<MI_TYPE_IQ4_NL>{}); break;
        case MI_TYPE_IQ4_XS: f(mi_type_c<MI_TYPE_IQ4_XS>{}); break;
        case MI_TYPE_F16: f(mi_type_c<MI_TYPE_F16>{}); break;
        case MI_TYPE_BF16: f(mi_type_c<MI_TYPE_BF16>{}); break;
        case MI_TYPE_F32: f(mi_type_c<MI_TYPE_F32>{}); break;
        default: MI_ASSERT(!"weight type outside the table");
    }
}
