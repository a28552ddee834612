// mi355x_kernels.h -- host-side launchers of the gfx950 kernels (internal to the backend).
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "mi355x_types.h"

// Activation columns of one mul_mat, quantized exactly as the reference CPU path quantizes
// them (vec_dot_type from_float, src/ggml.c:11952-11974), stored structure-of-arrays in HBM:
//   qs  [ncols][K]      int8 quants
//   d   [ncols][K/QK]   f32 block scale (Q8_0: the fp16-rounded d; Q8_K: f32 d)
//   s32 [ncols][K/32]   int16 sums of 32 quants (Q8_K; = bsums[2j] + bsums[2j+1]), or the fp16 bits of
//                       the block's s = d * sum(qs) (Q8_1, the vec_dot_type of Q4_1 / Q5_1: Q8_0 + s)
struct mi_act_q8 {
    int8_t * qs;
    float * d;
    int16_t * s32;
    int64_t K;
    int64_t ncols;
};

// Strided f32 activation source: column c = i1 + ne1*(i2 + ne2*i3) starts at
// base + i1*nb1 + i2*nb2 + i3*nb3 (elements along K contiguous).
struct mi_src_cols {
    const char * base;
    int64_t ne1, ne2, ne3;
    size_t nb1, nb2, nb3;
};

// GGML_OP_MUL_MAT_ID: the id table of an expert-routed mul_mat (ids == nullptr: a plain mul_mat).
// The weight-batch index is read by the kernels, never by the host. With it the batch coordinate
// (e, t), e < n_ids, t < ne12 takes its weight matrix from ids[e, t] (W + id * nb02), its
// activation column from index (e % ne11) + ne11 * t of the converted activations and its
// destination from e * nb1 + t * nb2. A pair whose id is outside [0, n_as) is skipped.
struct mi_mm_ids {
    const int32_t * ids = nullptr;  // ids[e, t] at (char *) ids + e * nb0 + t * nb1
    size_t nb0 = 0, nb1 = 0;
    int n_as = 0, n_ids = 0;
    // the pairs grouped by expert on the device (mi_mmid_group), or null: pairwise
    const int4 * chunks = nullptr;     // [mi_mmid_max_chunks] {expert, first, count <= chunk_cap (0: unused), 0}
    const int32_t * pairs = nullptr;   // pair indices e + n_ids * t, expert by expert, each list t-major
    int chunk_cap = 4;                 // pairs per chunk at most: 4 or 8 (columns per workgroup of the grouped GEMV)
};
// worst-case chunk count of a grouped MUL_MAT_ID: every expert's last chunk may be partial
inline int64_t mi_mmid_max_chunks(int64_t n_as, int64_t pairs, int cap) { return n_as + (pairs + cap - 1) / cap; }
constexpr int kMiMmidMaxExperts = 1024;  // mi_mmid_group keeps a counter per expert in LDS
// One launch, capturable: the counting sort of ggml_compute_forward_mul_mat_id (src/ggml.c:12169-12184)
// on the device. Fills chunks [mi_mmid_max_chunks(n_as, n_ids * n_tokens, id.chunk_cap)] and pairs [n_ids * n_tokens].
void mi_mmid_group(const mi_mm_ids & id, int64_t n_tokens, int4 * chunks, int32_t * pairs, hipStream_t s);

// Weight matrix / output description shared by the mul_mat launchers.
struct mi_mm_desc {
    const void * W;        // src0 data
    int type;              // ggml_type of src0
    int64_t K, N;          // ne00, ne01
    int64_t ne02, ne03;    // src0 batch dims (broadcast into src1's)
    size_t nb01, nb02, nb03;
    int64_t ne11, ne12, ne13;  // src1 columns / batch dims
    float * dst;
    size_t nb1, nb2, nb3;  // dst strides in bytes (nb0 == 4)
    mi_mm_ids id;          // MUL_MAT_ID (then ne02 = n_as, ne12 = n_tokens, ne03 = ne13 = 1)
};

// q: MI_ACT_Q8_0, MI_ACT_Q8_1 or MI_ACT_Q8_K
size_t mi_act_q8_bytes(int64_t K, int64_t ncols, mi_act_quant q);
mi_act_q8 mi_act_q8_carve(void * base, int64_t K, int64_t ncols, mi_act_quant q);

void mi_quantize_q8_0(const mi_src_cols & x, int64_t K, const mi_act_q8 & act, hipStream_t s);
void mi_quantize_q8_1(const mi_src_cols & x, int64_t K, const mi_act_q8 & act, hipStream_t s);
void mi_quantize_q8_K(const mi_src_cols & x, int64_t K, const mi_act_q8 & act, hipStream_t s);
// blocked: write the F16 prompt GEMMs' K-blocked layout [K/16][ncols][16] instead of [ncols][K];
// src_f16: the columns are f16 already (copied, not rounded)
void mi_convert_f16(const mi_src_cols & x, int64_t K, uint16_t * out, hipStream_t s, bool blocked = false, bool src_f16 = false);

// quantized weights x quantized activations (integer dot products), any number of columns
void mi_mul_mat_q(const mi_mm_desc & m, const mi_act_q8 & act, hipStream_t s);

// Decode-regime mul_mat with the activation quantizer fused in; one launch serves up to
// kMiMaxMembers independent mul_mats of identical weight type / shape (2-D weights, 2-D f32 src1
// with 16-byte aligned columns, contiguous f32 dst columns).
constexpr int kMiMaxMembers = 64;
struct mi_mmv_member {
    const void * W;
    const char * X;
    float * dst;
};
struct mi_mmv_group {
    int type;
    int n;                  // members in this launch
    int ncols;              // src1 columns (ne11), 1..8
    int blocks_per_member;  // set by the launcher
    int64_t rows_per_block; // set by the launcher
    int64_t K, N;
    size_t nb01;            // weight row stride (bytes)
    size_t xcol;            // src1 column stride (bytes)
    size_t ycol;            // dst column stride (bytes)
    int ord_rows = 0;       // reference order: rows per chain pass (0: one pass per 64-item chunk of a row)
    int ord_cs = 0;         // reference order: scratch words per (row, column)
    int ord_s = 0;          // reference order: Q4_0/Q8_0 lane-row stride in the scratch
    // the graph's following bias / residual / GELU and K/V row copies (one-member groups; same
    // fields and rounding as mi_f16_epilogue)
    struct epilogue {
        const float * bias = nullptr;
        const char * resid = nullptr;
        size_t resid_nb1 = 0;
        const uint16_t * gelu_table = nullptr;
        struct row_copy {
            int64_t row0 = 0, row1 = 0;
            char * ptr = nullptr;
            size_t col_stride = 0;
        } copy[2];
    } epi;
    // the graph's norm|rms_norm -> mul(g) -> add(b) producing src1, computed by the kernel from X
    // (one-member groups, K <= 768; same semantics as mi_norm_prologue)
    struct prologue {
        const float * g = nullptr;
        const float * b = nullptr;
        float eps = 0.0f;
        int mode = 0;  // 0 none, 1 norm, 2 rms_norm
    } pro;
    int pro_off = 0;   // set by the launcher: LDS byte offset of the normalized columns
    int q0r = 0;       // Q4_0 / Q8_0: every member's W is its 16-byte-aligned repacked copy (mi_planes_get), nb01 = K / 32 * the block's bytes
    int pro_q = 0;     // set by the launcher (g_mi_tuning.mmv_pro4): one Q8_K column's norm prologue quantizes from registers
    mi_mmv_member m[kMiMaxMembers];
    // GGML_OP_MUL_MAT_ID decode (behind m: the other fields keep their places; ncols == 1, no prologue / epilogue): ids_w != nullptr makes every
    // member's W a pointer to its int32 expert id in device memory; the kernel streams
    // ids_w + id * ids_nb02 and skips a member whose id is outside [0, ids_n_as)
    const void * ids_w = nullptr;
    size_t ids_nb02 = 0;
    int ids_n_as = 0;
};
bool mi_mmv_fused_supported(int type, int64_t K, int64_t ncols);
constexpr int64_t kMiMmvProMaxK = 768;  // norm prologue: the column is held in one wave's registers

// launch-shape knobs of the kernels (defaults tuned on MI355X; settable for A/B runs). Every field is
// a row of the knob table in mmv_fused.hip: set_tuning("<field>", v) and GGML_MI355X_<FIELD>=v pass
// the same range check.
struct mi_tuning {
    int mmv_blocks = 0;    // target resident workgroups for the fused GEMV (all members); 0: from the kernel's residency (hipOccupancy...) per instance
    int mmv_variant = 0;   // 10*prefetch_depth + {0: activations in VGPRs, 1: from LDS, 2: LDS + waves/EU cap}; 0: the per-type default
    int f16_variant = 0;   // decode F16 GEMV: 0 = 16 lanes per row (k_mmv_f16_w16), 1 = quad per row (k_mmv_f16_x)
    int f16_threads = 0;   // k_mmv_f16_w16 workgroup size override (0 = automatic)
    int mmq_variant = 0;   // exact prefill GEMMs: bits that move a launcher's decision to another column count (mi_mmq_variant_bits below; any other bit is refused); 0 = the defaults
    int attn_variant = 0;  // attention block: 0 = k_attn_fast where it fits, 1 = k_attn_ordered
    int mmv_order = -1;    // decode GEMVs (quantized and F16) and attention: 1 = the reference CPU's summation order (bit-identical,
                           // slower), 0 = tree sums, -1 (default) = per graph: 1 where a quantized MUL_MAT consumes a value the
                           // graph computes (its activation re-quantization would carry order differences forward), else 0
    int f16_waves = 0;     // fast F16 decode GEMV: target waves on the chip (0 = automatic)
    int f16_rgs = 0;       // fast F16 decode GEMV: row groups (4 rows) per workgroup (0 = automatic)
    int f16_ps_waves = 0;  // k_gemv_f16_ps (GEMV over summed partials): waves per workgroup, 2 / 4 / 8 (0 = automatic)
    int f16_norm_waves = 0;  // F16 GEMV, several columns with the norm prologue: waves per workgroup (0 = automatic)
    int planes = 0;        // long Q4_K prompts on repacked MFMA planes (mmq_planes.hip k_mmqr): 1 on, 0 off (default: slower than k_mmqt with HBM-streamed weights)
    int f16_nc = 10;       // F16 decode GEMVs: columns per workgroup at most (ones digit: plain, tens: norm prologue; 0: up to 8)
    int f16_bn = 5;        // F16 decode GEMVs, 2..8 columns with the norm prologue (K <= 1024) on k_gemv_f16_bn: 0 off, 1-5 shapes (default 5), +10 one column too
    int q40r = 1;          // tree-order Q4_0 decode GEMVs on the 16-byte-aligned repacked copy (mmq_planes.hip k_q40_repack, FmtQ0R): 1 on (default), 0 off
    int q80r = 1;          // tree-order Q8_0 decode GEMVs on the 16-byte-aligned repacked copy (k_q80_repack, FmtQ8R): 1 on (default), 0 off
    int mmv_pro4 = 1;      // decode GEMVs with the norm prologue, one Q8_K column: normalize and quantize in registers (norm_quant_prologue1): 1 (default), 0 through LDS
    int f16_mt = 1;        // tall F16 GEMVs (lm_head) of 2..8 columns, K <= 768, on the matrix cores (k_gemv_f16_mt): 1 on (default), 0 k_gemv_f16_tall
    int mmqt_short = 192;  // Q4_K prompts of 33..128 columns on k_mmqt (128 x 64 tiles) when a launch has at least this many of its workgroups (default 192; 0: never)
    int mmid_group = 1;    // MUL_MAT_ID of quantized experts: 1 = prompts from the measured crossover on (reference order: 8 tokens; tree order: never) run
                           // over the pairs grouped by expert on the device (mi_mmid_group; up to 4 gathered columns per workgroup), 0 = pair by pair;
                           // 4 / 8: grouped from 2 tokens on in either order with chunks of that many pairs (A/B timing)
    int mmid_stream = 8;   // MUL_MAT_ID of quantized experts: up to this many tokens run on the streaming decode kernel, a member per pair (0: never)
    int fuse_router = 1;   // a mixture-of-experts router chain (soft_max, argsort DESC, top-k view, get_rows, sum_rows, div; at most 64 experts) as one launch: 1 on (default), 0 off
    int ord_prefill_cols = INT_MAX;  // reference-order graphs: quantized prompt mul_mats of up to this many columns run as 8-column chunks of the
                           // reference-order streaming GEMV (ord_prefill_chunked in the backend); longer prompts take the MFMA GEMMs; 0: off
    int tree_prefill_cols = 0;  // tree-order graphs: the same chunks for prompts of up to this many columns (0: off)
};
// looks `name` up in the knob table; false: unknown name or a value outside the knob's range
bool mi_tuning_set(const char * name, int value);
// mmq_variant bits (mmq_exact.hip's two dispatch functions). All but kMmq0xRows2W8 make a kernel that the default
// decisions also reach run at another column count or tile count -- the tests reach k_mmqt / k_mmqw / k_mmqx /
// k_mmq0x with a 68-column prompt that way. Within a weight-format family every kernel keeps the family's canonical
// combine, so any choice gives the same bits. The values are fixed; set_tuning refuses any bit outside kMmqVariantMask.
enum mi_mmq_variant_bits : int {
    kMmqShortKernels = 16,       // the short-prompt kernels (k_mmqp / k_mmq0p) at any column count
    kMmqLongKernels = 128,       // the long prompts' decision at any column count (Q4_0 / Q8_0: k_mmq0x NR = 2, 64 x 128)
    kMmqHalfWidth = 1 << 16,     // k_mmqx / k_mmq0x: half-width workgroups (64 x 64 tiles, 4 waves)
    kMmqFullWidth = 1 << 17,     // Q4_K: no automatic half-width k_mmqx below 256 full tiles
    kMmq0xRows2 = 1 << 24,       // with kMmqLongKernels, Q4_0 / Q8_0: k_mmq0x NR = 2 even with kMmqHalfWidth
    kMmq0xRows2W8 = 1 << 25,     // with kMmqLongKernels, Q4_0 / Q8_0: k_mmq0x NR = 2 with 8 waves (64 x 256; never a default, see mmq0_group)
    kMmqxOnly = 1 << 28,         // Q4_K / Q5_K long prompts: k_mmqx instead of k_mmqt / k_mmqw
};
constexpr int kMmqVariantMask = kMmqShortKernels | kMmqLongKernels | kMmqHalfWidth | kMmqFullWidth | kMmq0xRows2 | kMmq0xRows2W8 | kMmqxOnly;
extern mi_tuning g_mi_tuning;
// the order of the graph being launched when mmv_order is -1 (set by the backend per graph)
extern thread_local int tl_mi_graph_order;
inline int mi_mmv_order() { return g_mi_tuning.mmv_order >= 0 ? g_mi_tuning.mmv_order : tl_mi_graph_order; }
// The kernel the launchers picked for the most recent MUL_MAT / MUL_MAT_ID launch (quantized, BF16 aside:
// every F16 selection site too -- mi_mul_mat_f16_fast, the ordered launchers, mi_mul_mat_f16p,
// mi_mul_mat_mmq, the generic mi_mul_mat_f16): a string that lives as long as the library, stored at each
// selection site (ggml_backend_mi355x_last_mul_mat_route; the tests assert that a forced route was taken).
// It names the kernel and the template arguments that select an instance, then in square brackets the
// launch geometry a knob moves: "k_gemv_f16<nc4,u2,one,jm0,epi1,xh0>[ks3,rgs1]". A replayed capture
// launches no kernel from the host and leaves it alone.
extern const char * g_mi_last_route;
inline void mi_route(const char * name) { g_mi_last_route = name; }
// the same with a name formatted on the first launch of `key` (unique per site and instance) and kept
void mi_route_fmt(uint32_t key, const char * fmt, ...) __attribute__((format(printf, 2, 3)));
size_t mi_mmv_fused_lds_bytes(int type, int64_t K, int64_t ncols);
void mi_mul_mat_q_fused(mi_mmv_group & g, hipStream_t s);
// its per-format launchers, specialized in mmv_fused_q2k.hip, _q3k, _q4k, _q5k, _q6k, _q40, _q80, _q41, _q50, _q51, _iq4nl, _iq4xs (one
// translation unit each, so that the formats build in parallel)
template <int T> void mi_mmv_launch(const mi_mmv_group & g, int variant, hipStream_t s);
// Batched (prefill) mul_mat of F16 weights on MFMA (mmq.hip): 2-D weights [K, N], `ncols` f16 activation
// columns xh in the K-blocked layout [K/16][ncols][16] (mi_convert_f16), dst columns of ycol bytes.
// K % 256 == 0, 16-byte aligned weight rows and dst columns.
bool mi_mmq_supported(int64_t K, size_t nb01, size_t ycol);
void mi_mul_mat_mmq(const void * W, size_t nb01, int64_t K, int64_t N, const uint16_t * xh, int64_t ncols, float * dst, size_t ycol,
                    hipStream_t s);
// 9..128 columns (k_mmf16p): 32 x 32 tiles, K split over a tile's 4 waves; the same operands
bool mi_mmf16p_supported(int64_t K, int64_t N, size_t nb01, int64_t ncols, size_t ycol);
void mi_mul_mat_f16p(const void * W, size_t nb01, int64_t K, int64_t N, const uint16_t * xh, int64_t ncols, float * dst, size_t ycol,
                     hipStream_t s);

// ---- exact-integer prefill GEMM for Q4_K / Q5_K (mmq_exact.hip) ----
// q8_K activation quants in the int8-MFMA layouts: xq [K/64][ncols][64] int8, xd [K/256][ncols]
// f32 scale, xu [K/256][ncols][16] f16 (S_j & 63, S_j >> 6; S_j = sum of the 32 quants of
// sub-block j) -- the bytes of quantize_row_q8_K_reference, rearranged
struct mi_act_mmx {
    int8_t * xq;
    float * xd;
    uint16_t * xu;
    int64_t K;
    int64_t ncols;
};
size_t mi_act_mmx_bytes(int64_t K, int64_t ncols);
mi_act_mmx mi_act_mmx_carve(void * base, int64_t K, int64_t ncols);
void mi_quantize_q8_K_mmx(const mi_src_cols & x, int64_t K, const mi_act_mmx & act, hipStream_t s);
// several activation sources (same K) quantized by one launch
constexpr int kMiMaxPrefillMembers = 16;
struct mi_mmx_qgroup {
    int n = 0;
    int64_t K = 0;
    struct member {
        mi_src_cols x;
        mi_act_mmx act;
        int64_t col_begin;  // set by the launcher
    } m[kMiMaxPrefillMembers];
};
void mi_quantize_q8_K_mmx_group(mi_mmx_qgroup & q, hipStream_t s);
// q8_0 activations (Q4_0 / Q8_0 weights) in the MFMA layout: xq [K/32][ncols][32] int8, xd
// [K/32][ncols] f32 (xu unused) -- the bytes of the AVX2 quantize_row_q8_0, rearranged
size_t mi_act_mmx0_bytes(int64_t K, int64_t ncols);
mi_act_mmx mi_act_mmx0_carve(void * base, int64_t K, int64_t ncols);
void mi_quantize_q8_0_mmx_group(mi_mmx_qgroup & q, hipStream_t s);
// src1 of the weight's vec_dot type (quantize.hip): GGML_OP_CPY F32 -> Q8_K / Q8_0 / Q8_1 rows in the
// reference block layouts (dst columns addressed like src1's), and such rows -> the GEMV's q8 SoA
// (act) or the prefill GEMMs' MFMA layout (mx); exactly one of act / mx non-null (Q8_1: act)
void mi_quantize_rows_q8(const mi_src_cols & x, int64_t K, mi_act_quant q, const mi_src_cols & dst, hipStream_t s);
void mi_q8_rows_to_act(const mi_src_cols & xs, int64_t K, mi_act_quant q, const mi_act_q8 * act, const mi_act_mmx * mx, hipStream_t s);
bool mi_mmqx_supported(int type, int64_t K, size_t ycol, int64_t ncols, size_t nb01);
// Independent Q4_K / Q5_K (q8_K activations) or Q4_0 / Q8_0 (q8_0 activations, mi_act_mmx0_*)
// mul_mats (same type, K and activation column count) in one launch:
// member i = 2-D weights [K, N_i] x act_i.ncols columns -> dst_i (column stride ycol_i bytes)
struct mi_mmx_member {
    const void * W;
    size_t nb01;
    int64_t N;
    mi_act_mmx act;
    float * dst;
    size_t ycol;
    int64_t tile_begin;  // set by the launcher
    const char * planes;  // Q4_K / Q5_K: the weights' repacked MFMA planes (mi_planes_get) or null
};
struct mi_mmx_group {
    int type = 0;
    int n = 0;
    int64_t K = 0;
    mi_mmx_member m[kMiMaxPrefillMembers];
};
void mi_mul_mat_mmqx_group(mi_mmx_group & g, hipStream_t s);
// one member
void mi_mul_mat_mmqx(int type, const void * W, size_t nb01, int64_t K, int64_t N, const mi_act_mmx & act, float * dst,
                     size_t ycol, hipStream_t s, const char * planes = nullptr);
// Repacked MFMA planes of Q4_K / Q5_K weights for long prompts (mmq_planes.hip): per 32-row tile
// and superblock the int8 planes q * (sc_j bit field) in v_mfma_i32_32x32x32_i8 operand order, the
// U operand [m_j, 64 m_j] and (d, dmin) -- a device-side copy kept next to the canonical blocks,
// which stay untouched (get_tensor, views, GET_ROWS, cpy see the reference bytes). mi_planes_get
// returns the planes of W (creating them with one repack launch on s when missing and s is not
// capturing), or null (disabled: GGML_MI355X_PLANES=0, unsupported shape, capture). Any write to
// weight memory must be followed by mi_planes_refresh over the written bytes (a repack launch on
// s for every overlapping entry; capturable); freeing the memory by mi_planes_drop.
constexpr int64_t kMiPlanesMinCols = 129;  // prompts of more columns take the planes kernel
// Types with mi_type().aligned_copy (Q4_0 / Q8_0, g_mi_tuning.q40r / q80r): the tree-order decode
// GEMV's 16-byte-aligned copy instead (k_q40_repack / k_q80_repack: per row the quants of every
// block, then their f16 scales; as many bytes a row as the canonical blocks).
const char * mi_planes_get(int type, const void * W, size_t nb01, int64_t K, int64_t N, hipStream_t s);
// the knob of a type's aligned copy (false: the type has none)
inline bool mi_aligned_copy_on(int type) {
    return mi_type(type).aligned_copy && (type == MI_TYPE_Q4_0 ? g_mi_tuning.q40r : g_mi_tuning.q80r) != 0;
}
void mi_planes_refresh(const void * lo, size_t bytes, hipStream_t s);
void mi_planes_drop(const void * lo, size_t bytes);
size_t mi_planes_count();
uint64_t mi_planes_generation();  // changes whenever a planes entry is created or dropped (graph keys)
size_t mi_planes_bytes();
// the planes kernel over a group whose members all carry planes (false: not applicable)
bool mi_mul_mat_mmqr_group(mi_mmx_group & g, hipStream_t s);

// ---- companion ops (ops.hip) ----
// a tensor view as the element-wise kernels see it: MI_TYPE_F32, MI_TYPE_F16 or MI_TYPE_I32 elements
struct mi_tensor_desc {
    char * data;
    int type;
    int64_t ne[4];
    size_t nb[4];
};
enum mi_elt_op { MI_OP_ADD, MI_OP_MUL, MI_OP_SUB, MI_OP_DIV, MI_OP_SCALE, MI_OP_GELU, MI_OP_SILU, MI_OP_CPY };
void mi_op_binary(const mi_tensor_desc & d, const mi_tensor_desc & a, const mi_tensor_desc & b, int op, hipStream_t s);
void mi_op_unary(const mi_tensor_desc & d, const mi_tensor_desc & a, int op, float p0, const uint16_t * table, hipStream_t s);
void mi_op_cpy(const mi_tensor_desc & d, const mi_tensor_desc & a, hipStream_t s);
// several independent copies (element i of a[c] -> element i of d[c]) in one launch
constexpr int kMiMaxCopies = 4;
void mi_op_cpy_multi(const mi_tensor_desc * d, const mi_tensor_desc * a, int count, hipStream_t s);
void mi_op_get_rows(const mi_tensor_desc & d, const mi_tensor_desc & a, const mi_tensor_desc & idx, hipStream_t s);
// d = get_rows(a, ia) + get_rows(b, ib) (1-D index vectors, f32 dst): the graph's two GET_ROWS and
// their ADD in one launch, each value as the separate nodes compute it
void mi_op_get_rows_add(const mi_tensor_desc & d, const mi_tensor_desc & a, const mi_tensor_desc & ia, const mi_tensor_desc & b,
                        const mi_tensor_desc & ib, hipStream_t s);
void mi_op_diag_mask(const mi_tensor_desc & d, const mi_tensor_desc & a, int n_past, float value, hipStream_t s);
// norm / rms_norm; g, b (optional, 1-D over ne0): the graph's following mul(., g) and add(., b)
void mi_op_norm(const mi_tensor_desc & d, const mi_tensor_desc & a, float eps, bool rms, const float * g, const float * b,
                hipStream_t s);
// rope f32 forward, modes 0/2; corr = ggml_rope_yarn_corr_dims() computed on the host; tab: the
// backend's host-built {cos, sin} table [tab_p][pairs] for positions < tab_p (or null)
void mi_op_rope(const mi_tensor_desc & d, const mi_tensor_desc & a, const int32_t * pos, int n_dims, int mode, float freq_base,
                float freq_scale, float ext_factor, float attn_factor, float corr0, float corr1, const float * tab, int tab_p,
                hipStream_t s);
// soft_max (max_bias 0); n_past >= 0 fuses the preceding scale(pre_scale) + diag_mask_inf(n_past)
void mi_op_soft_max(const mi_tensor_desc & d, const mi_tensor_desc & a, const mi_tensor_desc & mask, float scale,
                    const uint16_t * exp_table, float pre_scale, int n_past, hipStream_t s);

// ---- mixture-of-experts router ops (router.hip) ----
// sum_rows f32 (src/ggml.c:10159-10192): d[0, i1, i2, i3] = the row's sequential double sum, rounded once
void mi_op_sum_rows(const mi_tensor_desc & d, const mi_tensor_desc & a, hipStream_t s);
// argsort f32 -> i32 (src/ggml.c:15064-15105), ne0 <= kMiArgsortMaxRow: the permutation the reference's
// exchange sort leaves, ties included. Row r of src / dst at r * nb[1], as the reference addresses them.
constexpr int kMiArgsortMaxRow = 1024;
void mi_op_argsort(const mi_tensor_desc & d, const mi_tensor_desc & a, bool descending, hipStream_t s);
// soft_max -> argsort DESC -> first k -> get_rows of the probabilities -> (sum_rows -> div) of one
// router, one wave per token, every tensor as its own node would write it. All contiguous.
constexpr int kMiRouterMaxExperts = 64;
struct mi_router_desc {
    const float * logits;  // [n_expert, T]
    float * probs;         // [n_expert, T]
    int32_t * sorted;      // [n_expert, T] argsort rows: the first n_sorted entries of each are written
    float * weights;       // [k, T] probs[sorted[j, t], t]
    float * sums;          // [T], or null: no normalisation tail
    float * normed;        // [k, T] weights / sums
    int n_expert, k, n_sorted;  // n_sorted = k, or n_expert where the argsort has other readers
    int64_t T;
};
void mi_router_fused(const mi_router_desc & r, const uint16_t * exp_table, hipStream_t s);

// ---- GGML_OP_SSM_CONV / GGML_OP_SSM_SCAN (ssm.hip; src/ggml.c:16311-16543) ----
// All f32 but sq (i32 [n_kv, n_tokens], read by the kernels: a token whose sq[0] is outside [0, n_kv) is
// skipped). d is 1-D: the outputs [d_inner, n_tokens], then the new states of every sequence. One launch each.
// conv: s [d_conv - 1, d_inner, n_kv] (rows contiguous), x [d_inner, n_tokens] (nb0 == 4), c [d_conv, d_inner]
// contiguous, d_conv in 2..8; the states in d are d_conv wide
bool mi_ssm_conv_width_ok(int64_t d_conv);
void mi_op_ssm_conv(const mi_tensor_desc & d, const mi_tensor_desc & s, const mi_tensor_desc & x, const mi_tensor_desc & c,
                    const mi_tensor_desc & sq, hipStream_t st);
// scan: s [d_state, d_inner, n_kv] and x [d_inner, n_tokens] contiguous; dt like x, A [d_state, d_inner] and
// B / C [d_state, n_tokens] with nb0 == 4 and any row stride; any d_state >= 1 (16: the fast kernel)
void mi_op_ssm_scan(const mi_tensor_desc & d, const mi_tensor_desc & s, const mi_tensor_desc & x, const mi_tensor_desc & dt,
                    const mi_tensor_desc & A, const mi_tensor_desc & B, const mi_tensor_desc & C, const mi_tensor_desc & sq,
                    hipStream_t st);

// ---- GGML_OP_FLASH_ATTN_EXT (flash_attn.hip; src/ggml.c:15572-15751) ----
// q f32 [D, N, nh, ne3] (nb0 == 4), k / v f16 [D, kv, nh_k / nh_v, ne3_k / ne3_v] (nb0 == 2), mask f16
// rows of nbm1 bytes or null, dst f32 [D, nh, N, ne3] contiguous.
struct mi_fa_desc {
    const char * q;
    const char * k;
    const char * v;
    const char * mask;
    float * dst;
    float * part;  // split partials, mi_fa_part_bytes (null when mi_fa_splits == 1)
    int D, N, nh, ne3, kv;
    int nh_k, nh_v, ne3_k, ne3_v;
    size_t nbq1, nbq2, nbq3, nbk1, nbk2, nbk3, nbv1, nbv2, nbv3, nbm1;
    float scale, max_bias;
};
bool mi_fa_head_size_ok(int64_t D);
// the number of workgroups the KV range is split over: a pure function of the shape
int mi_fa_splits(const mi_fa_desc & d);
size_t mi_fa_part_bytes(const mi_fa_desc & d);
// one launch, or the split kernel and its combine; returns the number of launches
int mi_flash_attn_ext(const mi_fa_desc & d, hipStream_t s);

// Decode-regime F16 mul_mat (2-D weights, few f32 src1 columns of contiguous K) that converts the
// activations itself and applies the graph's following bias add / residual add / GELU.
struct mi_f16_epilogue {
    const float * bias = nullptr;        // [N] f32, or null
    const char * resid = nullptr;        // [N, ncols] f32 (row stride resid_nb1), or null
    size_t resid_nb1 = 0;
    const uint16_t * gelu_table = nullptr;  // fp16 GELU table (applied after bias), or null
    // up to two extra destinations of output row ranges (the graph's following CPY of a row view of
    // the output, e.g. GPT-2's K/V cache writes): element (row, col) with row0 <= row < row1 is
    // also stored at ptr + col * col_stride + (row - row0) * 4
    struct row_copy {
        int64_t row0 = 0, row1 = 0;
        char * ptr = nullptr;
        size_t col_stride = 0;
    } copy[2];
};
// optional prologue: src1 = add(mul(norm|rms_norm(x, eps), g), b) computed in the kernel from x
struct mi_norm_prologue {
    const float * g = nullptr;  // [K] or null
    const float * b = nullptr;  // [K] or null
    float eps = 0.0f;
    int mode = 0;               // 0 none, 1 norm, 2 rms_norm
    // the norm's input as partial sums (mi_attn_proj's output; fast F16 path, one column only):
    // x = sum_{p < nparts} parts[p][0 .. K), and the first workgroup stores x to `store`
    const float * parts = nullptr;
    int nparts = 0;
    float * store = nullptr;
};
bool mi_mul_mat_f16_fused_supported(int64_t K, int64_t ncols);
// xh: optional f16 [ncols][K] activations already converted (then x is not read)
void mi_mul_mat_f16_fused(const void * W, size_t nb01, int64_t K, int64_t N, const mi_src_cols & x, const uint16_t * xh,
                          int64_t ncols, float * dst, size_t ycol, const mi_f16_epilogue & e, const mi_norm_prologue & pro,
                          hipStream_t s);

// the same in tree order (mmv_f16.hip; the fast F16 decode mode, mmv_order 0): 1..8 columns,
// K % 8 == 0, 16-byte aligned activation columns (or xh), norm prologue for K <= 3072
bool mi_mul_mat_f16_fast_supported(int64_t K, int64_t ncols, const mi_src_cols & x, const uint16_t * xh, const mi_norm_prologue & pro);
void mi_mul_mat_f16_fast(const void * W, size_t nb01, int64_t K, int64_t N, const mi_src_cols & x, const uint16_t * xh, int64_t ncols,
                         float * dst, size_t ycol, const mi_f16_epilogue & e, const mi_norm_prologue & pro, hipStream_t s);

// attention of the GPT-2 graph (KQ, scale, causal mask, soft_max, KQV, merge) in one launch,
// bit-identical to the separate nodes. Strides in bytes; element (i0, i1, i2) at base + sum i*nb.
struct mi_attn_desc {
    const char * q;   // Q [D, N, H]
    size_t q_nb[3];
    const char * k;   // K [D, n_kv, Hk]
    size_t k_nb[3];
    const char * v;   // V_trans [n_kv, D, Hk]
    size_t v_nb[3];
    char * out;       // KQV (d, t, h) destination
    size_t o_nb[3];
    int D, N, H, n_kv, r2;  // r2 = H / Hk
    int n_past;             // diag_mask_inf n_past
    float pre_scale;        // ggml_scale factor
    float sm_scale;         // soft_max scale (op_params[0])
    const char * mask = nullptr;  // ADD(scale(KQ), mask) form: F32 mask [n_kv, N] added after the
    size_t mask_nb1 = 0;          // pre-scale (n_past then disables the causal mask)
};
bool mi_attn_supported(int D, int n_kv);
// mmv_order 1 (or attn_variant 1): the reference's summation order, bit-identical; otherwise the
// tree-order kernel of attn_fast.hip where it applies (mi_attn_tree_supported)
void mi_attn_ordered(const mi_attn_desc & a, const uint16_t * exp_table, hipStream_t s);
bool mi_attn_tree_supported(const mi_attn_desc & a);
void mi_attn_tree(const mi_attn_desc & a, hipStream_t s);
// one decode token's attention fused with the F16 output projection W [K = D H, N] that consumes
// it, plus the projection's bias and residual ADDs: parts[h][i] = W[i, hD .. hD + D) . o_h (head 0
// also + bias[i] + resid[i]); sum_h parts[h] (head order) is the projection's output
struct mi_attn_proj_desc {
    const uint8_t * W;
    size_t nb01;
    int64_t N;
    const float * bias;   // [N]
    const float * resid;  // [N]
    float * parts;        // [H][N]
};
bool mi_attn_proj_supported(const mi_attn_desc & a, int64_t K, int64_t N, size_t nb01, const void * W);
void mi_attn_proj(const mi_attn_desc & a, const mi_attn_proj_desc & p, hipStream_t s);
// out[i] = sum_{h < nparts} parts[h][i], in h order
void mi_sum_parts(float * out, const float * parts, int nparts, int64_t n, hipStream_t s);

// f16 weights x f16-rounded activations
void mi_mul_mat_f16(const mi_mm_desc & m, const uint16_t * xh, hipStream_t s);
// bf16 weights x bf16 activations (mm_bf16.hip). mi_convert_bf16: src1 columns of src_type MI_TYPE_F32 /
// MI_TYPE_F16 (rounded with ggml_fp32_to_bf16's bits) or MI_TYPE_BF16 (copied) -> bf16 rows [ncols][K].
// mi_mul_mat_bf16: xb those rows; any K, row alignment, column count, weight batch and MUL_MAT_ID;
// mmv_order 1: ggml_vec_dot_bf16's bits
void mi_convert_bf16(const mi_src_cols & x, int64_t K, uint16_t * out, int src_type, hipStream_t s);
void mi_mul_mat_bf16(const mi_mm_desc & m, const uint16_t * xb, hipStream_t s);
// f32 x f32, both operands arbitrarily strided (src1 described by x, src0 by m.nb0x)
void mi_mul_mat_f32(const mi_mm_desc & m, const mi_src_cols & x, hipStream_t s);
