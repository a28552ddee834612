// mul_mat.cpp -- GGML_OP_MUL_MAT and GGML_OP_MUL_MAT_ID of the MI355X backend: the activation cache,
// the choice of kernel per node (src/ggml-cuda.cu:2156-2308 analogue), weights split over devices
// (:1360-1647 analogue) and the launches that serve several nodes at once.

#include "mi_backend.h"

#include <mutex>

// ---------------------------------------------------------------------------------------------
// GGML_OP_MUL_MAT
// ---------------------------------------------------------------------------------------------

// the activations of weight type t as its GEMV reads them: q8 SoA, or f16 / bf16 rows
mi_act_format act_format_of(ggml_type t) {
    const mi_act_quant q = mi_type(t).act;
    return {q, q == MI_ACT_F16 || q == MI_ACT_BF16 ? MI_LAYOUT_ROWS : MI_LAYOUT_SOA};
}

static mi_act_mmx mmx_carve(mi_act_quant q, void * base, int64_t K, int64_t ncols) {
    return q == MI_ACT_Q8_K ? mi_act_mmx_carve(base, K, ncols) : mi_act_mmx0_carve(base, K, ncols);
}

// the only function that knows sizes
size_t act_bytes(mi_act_format f, int64_t K, int64_t ncols) {
    switch (f.layout) {
        case MI_LAYOUT_SOA: return mi_act_q8_bytes(K, ncols, f.quant);
        case MI_LAYOUT_MFMA: return f.quant == MI_ACT_Q8_K ? mi_act_mmx_bytes(K, ncols) : mi_act_mmx0_bytes(K, ncols);
        case MI_LAYOUT_ROWS:
        case MI_LAYOUT_BLOCKED: return (size_t) K * ncols * 2;
    }
    return 0;
}

mi_src_cols src_cols(const ggml_tensor * t) {
    mi_src_cols x;
    x.base = (const char *) t->data;
    x.ne1 = t->ne[1];
    x.ne2 = t->ne[2];
    x.ne3 = t->ne[3];
    x.nb1 = t->nb[1];
    x.nb2 = t->nb[2];
    x.nb3 = t->nb[3];
    return x;
}

// Converted activations for (src1, format), reused by later mul_mats of the same graph that read
// the same, unmodified src1 (Q/K/V or gate/up projections share their input).
static void * find_activations(const mi_backend_ctx * ctx, const ggml_tensor * src1, mi_act_format f) {
    for (const auto & e : ctx->act_cache) {
        if (e.data == src1->data && e.format == f && memcmp(e.ne, src1->ne, sizeof(e.ne)) == 0 &&
            memcmp(e.nb, src1->nb, sizeof(e.nb)) == 0) {
            return e.dev;
        }
    }
    return nullptr;
}

static void cache_activations(mi_backend_ctx * ctx, const ggml_tensor * src1, mi_act_format f, void * dev) {
    mi_act_cache_entry e;
    e.data = src1->data;
    e.nbytes = ggml_nbytes(src1);
    e.format = f;
    memcpy(e.ne, src1->ne, sizeof(e.ne));
    memcpy(e.nb, src1->nb, sizeof(e.nb));
    e.dev = dev;
    ctx->act_cache.push_back(e);
}

static void * get_activations(mi_backend_ctx * ctx, const ggml_tensor * src1, mi_act_format f, int64_t K) {
    if (void * hit = find_activations(ctx, src1, f)) return hit;
    const int64_t ncols = src1->ne[1] * src1->ne[2] * src1->ne[3];
    void * dev = scratch_take(ctx, act_bytes(f, K, ncols));
    const mi_src_cols x = src_cols(src1);
    if (q8_quant_of(src1->type) != MI_ACT_NONE) {
        // already quantized by the reference's rules (e.g. a CPY F32 -> Q8_K): re-laid out only
        MI_ASSERT(q8_quant_of(src1->type) == f.quant);
        MI_ASSERT(f.layout == MI_LAYOUT_SOA || (f.layout == MI_LAYOUT_MFMA && f.quant != MI_ACT_Q8_1));
        if (f.layout == MI_LAYOUT_MFMA) {
            const mi_act_mmx mx = mmx_carve(f.quant, dev, K, ncols);
            mi_q8_rows_to_act(x, K, f.quant, nullptr, &mx, ctx->stream);
        } else {
            const mi_act_q8 act = mi_act_q8_carve(dev, K, ncols, f.quant);
            mi_q8_rows_to_act(x, K, f.quant, &act, nullptr, ctx->stream);
        }
    } else if (f.layout == MI_LAYOUT_MFMA) {
        mi_mmx_qgroup q;
        q.n = 1;
        q.K = K;
        q.m[0].x = x;
        q.m[0].act = mmx_carve(f.quant, dev, K, ncols);
        if (f.quant == MI_ACT_Q8_K) mi_quantize_q8_K_mmx_group(q, ctx->stream);
        else mi_quantize_q8_0_mmx_group(q, ctx->stream);
    } else if (f.layout == MI_LAYOUT_SOA) {
        const mi_act_q8 act = mi_act_q8_carve(dev, K, ncols, f.quant);
        if (f.quant == MI_ACT_Q8_K) mi_quantize_q8_K(x, K, act, ctx->stream);
        else if (f.quant == MI_ACT_Q8_1) mi_quantize_q8_1(x, K, act, ctx->stream);
        else mi_quantize_q8_0(x, K, act, ctx->stream);
    } else if (f.quant == MI_ACT_BF16) {
        // bf16 rows (ggml_fp32_to_bf16_row's bits; a BF16 src1 is copied as it lies): never the f16 converter
        MI_ASSERT(f.layout == MI_LAYOUT_ROWS);
        mi_convert_bf16(x, K, (uint16_t *) dev, (int) src1->type, ctx->stream);
    } else {
        MI_ASSERT(f.quant == MI_ACT_F16);
        mi_convert_f16(x, K, (uint16_t *) dev, ctx->stream, f.layout == MI_LAYOUT_BLOCKED, src1->type == GGML_TYPE_F16);
    }
    ctx->last_launches++;
    cache_activations(ctx, src1, f, dev);
    return dev;
}

void invalidate_activations(mi_backend_ctx * ctx, const ggml_tensor * written) {
    const char * lo = (const char *) written->data;
    const char * hi = lo + ggml_nbytes(written);
    // a node writing into memory that repacked planes mirror (weights written through a view, or a
    // reused compute-buffer region that once held a Q4_K leaf) renews the planes over it
    if (mi_planes_count() > 0) mi_planes_refresh(lo, (size_t) (hi - lo), ctx->stream);
    auto & c = ctx->act_cache;
    c.erase(std::remove_if(c.begin(), c.end(), [&](const mi_act_cache_entry & e) {
                const char * elo = (const char *) e.data;
                return elo < hi && lo < elo + e.nbytes;
            }),
            c.end());
}

// a batched (prompt) GEMM applies: more than 8 columns of plain 2-D operands that the F16 GEMMs
// (mmq.hip) resp. the exact int8 GEMMs (mmq_exact.hip) accept. Every other weight type, and a
// quantized shape the exact GEMM refuses (a row stride that is no multiple of 16 bytes, say), runs
// the prompt on its GEMV in 8-column chunks.
static bool mm_batched(const mi_mm_desc & m, const ggml_tensor * src1) {
    if (mi_env().no_mmq || src1->ne[1] <= 8 || m.ne02 != 1 || m.ne03 != 1 || m.ne12 != 1 || m.ne13 != 1 || ((uintptr_t) m.W % 16) != 0) return false;
    if (m.type == GGML_TYPE_F16) return mi_mmq_supported(m.K, m.nb01, m.nb1);
    return mi_mmqx_supported(m.type, m.K, m.nb1, src1->ne[1], m.nb01);
}

// The activation format mul_mat_run converts src1 to for this mul_mat (quant MI_ACT_NONE, F32
// weights: src1 is read as it lies). Batched (mm_batched): the exact-integer int8 GEMMs' MFMA layouts
// for Q4_K / Q5_K / Q4_0 / Q8_0 prompts, the K-blocked f16 layout for F16 prompts. Everything else: the
// weight type's own format (q8 SoA, f16 / bf16 rows) at any column count; the quantized GEMVs run a
// prompt in 8-column chunks.
static mi_act_format mm_act_format(const mi_mm_desc & m, const ggml_tensor * src1) {
    mi_act_format f = act_format_of((ggml_type) m.type);
    if (mm_batched(m, src1)) f.layout = f.quant == MI_ACT_F16 ? MI_LAYOUT_BLOCKED : MI_LAYOUT_MFMA;
    return f;
}

// A 2-D graph leaf (a weight: never a tensor a node of the graph writes) in one of this backend's own
// device buffers: what a repacked copy may mirror. Host and peer memory have write paths (host-buffer
// set/clear, peer copies) that do not renew the copies. Within a device buffer every write path renews
// them: set/get/cpy/clear (sync and async) and any graph node whose output overlaps an entry
// (invalidate_activations), so a compute buffer's reused memory is covered too
static bool own_device_leaf(const mi_backend_ctx * ctx, const ggml_tensor * a) {
    if (a->op != GGML_OP_NONE || a->ne[2] != 1 || a->ne[3] != 1 || is_split_tensor(a)) return false;
    const ggml_backend_buffer_t buf = a->view_src ? a->view_src->buffer : a->buffer;
    return buffer_is_mi355x(buf) && ((mi_buffer_ctx *) buf->context)->device == ctx->device;
}

// the repacked MFMA planes of the long Q4_K / Q5_K prompts' weights (before any capture: creating
// them allocates)
const char * planes_of(mi_backend_ctx * ctx, const ggml_tensor * a, const ggml_tensor * b) {
    if (!g_mi_tuning.planes || !mi_type(a->type).planes || b->ne[1] * b->ne[2] * b->ne[3] < kMiPlanesMinCols || !own_device_leaf(ctx, a))
        return nullptr;
    return mi_planes_get(a->type, a->data, a->nb[1], a->ne[0], a->ne[1], ctx->stream);
}

// The 16-byte-aligned copy of a Q4_0 / Q8_0 weight for the tree-order decode GEMV (mmq_planes.hip
// k_q40_repack / k_q80_repack; created before any capture, renewed by the same write paths as the planes)
const char * q40r_of(mi_backend_ctx * ctx, const ggml_tensor * a) {
    if (!mi_aligned_copy_on(a->type) || !own_device_leaf(ctx, a)) return nullptr;
    return mi_planes_get(a->type, a->data, a->nb[1], a->ne[0], a->ne[1], ctx->stream);
}

// A Q4_0 / Q8_0 decode group in tree order on the repacked copies (FmtQ0R / FmtQ8R): every member's
// weight must have one, else the canonical blocks (FmtQ0Pair / FmtQ0<true>) -- the same bits
void q40r_apply(mi_backend_ctx * ctx, mi_mmv_group & g, const ggml_tensor * const * w) {
    // (one column: with two, the aligned copy measured 2-3 % slower, profiles/r06s2_q40r_ab.txt)
    if (!mi_aligned_copy_on(g.type) || g.ncols != 1 || mi_mmv_order() != 0 ||
        (g.type == GGML_TYPE_Q4_0 && g_mi_tuning.mmv_variant % 10 == 1)) return;
    const void * p[kMiMaxMembers];
    for (int m = 0; m < g.n; m++) {
        p[m] = q40r_of(ctx, w[m]);
        if (!p[m]) return;
    }
    for (int m = 0; m < g.n; m++) g.m[m].W = p[m];
    g.nb01 = (size_t) (g.K / mi_type(g.type).blck * mi_type(g.type).bytes);
    g.q0r = 1;
}

// The fields that the members of a streaming-GEMV launch share: weights shaped and typed as w, ncols
// activation columns x_stride bytes apart, output columns out_stride bytes apart. The caller sets n
// and fills the members; the aligned copies (q40r_apply) are a separate step, taken by the decode
// groups only -- the chunked prompts and MUL_MAT_ID stream the canonical blocks.
void mmv_group_for(mi_mmv_group & g, const ggml_tensor * w, size_t x_stride, int ncols, size_t out_stride) {
    g.type = w->type;
    g.ncols = ncols;
    g.K = w->ne[0];
    g.N = w->ne[1];
    g.nb01 = w->nb[1];
    g.xcol = x_stride;
    g.ycol = out_stride;
}

// The descriptor of the mul_mat of (src0, src1) with src0's rows taken from (W, N) and the output
// written at out (column strides nb1..nb3). MUL_MAT_ID: src0 the expert stack, src1 its b.
static mi_mm_desc mm_desc(const ggml_tensor * src0, const void * W, int64_t N, const ggml_tensor * src1, float * out, size_t nb1, size_t nb2,
                          size_t nb3) {
    mi_mm_desc m{};
    m.W = W;
    m.type = src0->type;
    m.K = src0->ne[0];
    m.N = N;
    m.ne02 = src0->ne[2];
    m.ne03 = src0->ne[3];
    m.nb01 = src0->nb[1];
    m.nb02 = src0->nb[2];
    m.nb03 = src0->nb[3];
    m.ne11 = src1->ne[1];
    m.ne12 = src1->ne[2];
    m.ne13 = src1->ne[3];
    m.dst = out;
    m.nb1 = nb1;
    m.nb2 = nb2;
    m.nb3 = nb3;
    return m;
}

// The mul_mat of (src0, src1) with src0's rows taken from (W, N) and the output written at out
// (column strides nb1..nb3): op_mul_mat runs the whole node through it, the split-buffer path
// (op_mul_mat_split) each device's row slice.
static void mul_mat_run(mi_backend_ctx * ctx, const ggml_tensor * src0, const void * W, int64_t N, const ggml_tensor * src1,
                        float * out, size_t nb1, size_t nb2, size_t nb3) {
    MI_ASSERT(src1->type == GGML_TYPE_F32 || ((src1->type == GGML_TYPE_F16 || src1->type == GGML_TYPE_BF16) && src0->type == src1->type) ||
              src1->type == q8_src1_type(src0->type));
    MI_ASSERT(src0->nb[0] == ggml_type_size(src0->type));
    MI_ASSERT(src1->nb[0] == ggml_type_size(src1->type));
    MI_ASSERT(src0->ne[0] == src1->ne[0]);
    MI_ASSERT(src1->ne[2] % src0->ne[2] == 0 && src1->ne[3] % src0->ne[3] == 0);

    const mi_mm_desc m = mm_desc(src0, W, N, src1, out, nb1, nb2, nb3);
    const mi_act_format f = mm_act_format(m, src1);
    if (f.quant == MI_ACT_NONE) {
        MI_ASSERT(src0->type == GGML_TYPE_F32);
        mi_mul_mat_f32(m, src_cols(src1), ctx->stream);
    } else {
        const int64_t ncols = src1->ne[1] * src1->ne[2] * src1->ne[3];
        void * xa = get_activations(ctx, src1, f, m.K);
        const uint16_t * xh = (const uint16_t *) xa;
        switch (f.layout) {
            case MI_LAYOUT_SOA:  // the GEMVs, at any column count
                mi_mul_mat_q(m, mi_act_q8_carve(xa, m.K, ncols, f.quant), ctx->stream);
                break;
            case MI_LAYOUT_MFMA:  // Q4_K / Q5_K / Q4_0 / Q8_0: the exact-integer int8 MFMA GEMMs (mmq_exact.hip)
                mi_mul_mat_mmqx(m.type, m.W, m.nb01, m.K, m.N, mmx_carve(f.quant, xa, m.K, ncols), m.dst, m.nb1, ctx->stream,
                                W == src0->data && N == src0->ne[1] ? planes_of(ctx, src0, src1) : nullptr);
                break;
            case MI_LAYOUT_ROWS:
            case MI_LAYOUT_BLOCKED:
                if (f.quant == MI_ACT_BF16) {
                    // BF16 weights: their own kernels at any column count and shape (mm_bf16.hip)
                    mi_mul_mat_bf16(m, xh, ctx->stream);
                } else if (f.layout == MI_LAYOUT_BLOCKED && mi_mmf16p_supported(m.K, m.N, m.nb01, ncols, m.nb1)) {
                    // F16 weights, a short prompt: 32 x 32 tiles with the K split over each tile's 4 waves
                    mi_mul_mat_f16p(m.W, m.nb01, m.K, m.N, xh, ncols, m.dst, m.nb1, ctx->stream);
                } else if (f.layout == MI_LAYOUT_BLOCKED) {
                    mi_mul_mat_mmq(m.W, m.nb01, m.K, m.N, xh, ncols, m.dst, m.nb1, ctx->stream);
                } else {
                    mi_mul_mat_f16(m, xh, ctx->stream);  // f16 rows of a mul_mat that is not batched: the F16 GEMV
                }
                break;
        }
    }
    ctx->last_launches++;
}

// the mul_mat descriptor of a whole MUL_MAT node (as mul_mat_run builds it)
static mi_mm_desc mm_desc_of(const ggml_tensor * node) {
    return mm_desc(node->src[0], node->src[0]->data, node->src[0]->ne[1], node->src[1], (float *) node->data, node->nb[1], node->nb[2], node->nb[3]);
}

static void op_mul_mat(mi_backend_ctx * ctx, ggml_tensor * dst) {
    MI_ASSERT(dst->nb[0] == sizeof(float));
    const ggml_tensor * src0 = dst->src[0];
    mul_mat_run(ctx, src0, src0->data, src0->ne[1], dst->src[1], (float *) dst->data, dst->nb[1], dst->nb[2], dst->nb[3]);
}

// the streaming GEMV's weight alignment: a 16-byte tensor base and rows of the type's mmv_align
// (16 bytes, Q6_K 2: mi355x_types.h); only for types mi_mmv_fused_supported accepts
static bool fused_weight_aligned(const ggml_tensor * a) {
    return (uintptr_t) a->data % 16 == 0 && a->nb[1] % mi_type(a->type).mmv_align == 0;
}

// The eligibility tests of this file (fused_mv_eligible, ord_prefill_chunked, prefill_mmx_format,
// mmid_stream_eligible) and try_fuse_f16_gemv (fusion.cpp) are written with plain_2d_operands,
// fused_weight_aligned and f32_cols_aligned; where one asks for more or less, it says so.
bool fused_mv_eligible(const ggml_tensor * n) {
    if (n->op != GGML_OP_MUL_MAT || is_split_tensor(n->src[0])) return false;
    const ggml_tensor * a = n->src[0];
    const ggml_tensor * b = n->src[1];
    if (b->type != GGML_TYPE_F32 || !mi_mmv_fused_supported(a->type, a->ne[0], b->ne[1])) return false;
    return plain_2d_operands(n) && fused_weight_aligned(a) && f32_cols_aligned(b);
}

static bool same_group_shape(const ggml_tensor * x, const ggml_tensor * y) {
    const ggml_tensor * xa = x->src[0];
    const ggml_tensor * ya = y->src[0];
    return xa->type == ya->type && xa->ne[0] == ya->ne[0] && xa->ne[1] == ya->ne[1] && xa->nb[1] == ya->nb[1] &&
           x->src[1]->ne[1] == y->src[1]->ne[1] && x->src[1]->nb[1] == y->src[1]->nb[1] && x->nb[1] == y->nb[1];
}

// ---------------------------------------------------------------------------------------------
// GGML_OP_MUL_MAT_ID (src/ggml.c:4852-4897, 12099-12279): dst[:, e, t] = as[:, :, ids[e, t]] . b[:, e % ne11, t]
// ---------------------------------------------------------------------------------------------
//
// The ids stay in device memory: every kernel looks its expert up itself, so the node is a fixed
// sequence of launches whatever the ids hold (stream capture, graph replay with new ids).
//   one token (mmid_stream: up to that many), quantized experts of streaming shape: one grouped
//     k_mmv_stream launch, a member per pair (the decode hot path; it quantizes b itself)
//   otherwise b is converted once through get_activations (gate and up of one block share the
//     copy) and the generic GEMVs run pair by pair, or, for quantized experts from
//     mmid_group_min_tokens() tokens on (mmid_group 1), over the pairs grouped by expert on the
//     device: up to 4 gathered columns per workgroup, each expert's weights read once per 4 pairs.

// pairs grouped by expert from this many tokens on (tools/mmid_gemv.py, profiles/mmid_gemv.txt, Q4_K
// 4096 x 14336, 2 of 8 experts): the reference-order GEMV (8 rows per wave) in chunks of 4 pairs is
// 0.90x the pairwise time at 8 tokens, 0.78x at 16, 0.57x at 512 (1.16x at 2); the tree-order GEMV
// (a wave per row: 139 VGPRs at 4 columns, ~240 at 8) never gained (1.05x at 512, 1.95x at 2)
static int64_t mmid_group_min_tokens() { return mi_mmv_order() == 1 ? 8 : INT64_MAX; }

size_t mmid_tables_bytes(int64_t n_as, int64_t pairs) {
    return align_up((size_t) mi_mmid_max_chunks(n_as, pairs, 4) * sizeof(int4)) + align_up((size_t) pairs * sizeof(int32_t));
}

// The operands are 3-D here (op_mul_mat_id asserts their element strides), so the alignment is asked
// of every expert matrix (fused_weight_aligned on the stack's base, and the expert stride) and of
// every token's columns (f32_cols_aligned, and the token stride).
static bool mmid_stream_eligible(const ggml_tensor * n) {
    const ggml_tensor * as = n->src[0], * b = n->src[1], * ids = n->src[2];
    if (mi_env().no_fused_mmv || b->ne[2] > g_mi_tuning.mmid_stream || ids->ne[0] * b->ne[2] > kMiMaxMembers) return false;
    if (!mi_mmv_fused_supported(as->type, as->ne[0], 1)) return false;
    if (!fused_weight_aligned(as) || as->nb[2] % 16 != 0) return false;
    return f32_cols_aligned(b) && b->nb[2] % 16 == 0 && ids->nb[0] == sizeof(int32_t);
}

void op_mul_mat_id(mi_backend_ctx * ctx, ggml_tensor * dst) {
    const ggml_tensor * as = dst->src[0], * b = dst->src[1], * ids = dst->src[2];
    // (the scheduler does not consult supports_op: anything it refuses stops here)
    MI_ASSERT(ids && ids->type == GGML_TYPE_I32 && ids->ne[2] == 1 && ids->ne[3] == 1);
    MI_ASSERT(mm_src0_supported(as->type) && as->nb[0] == ggml_type_size(as->type) && as->ne[3] == 1);
    MI_ASSERT(!is_split_tensor(as) && "MUL_MAT_ID: experts in a split buffer are not supported");
    MI_ASSERT(b->type == GGML_TYPE_F32 && b->nb[0] == sizeof(float) && b->ne[3] == 1 && "MUL_MAT_ID: src1 must be F32");
    MI_ASSERT(as->ne[0] == b->ne[0] && ids->ne[1] == b->ne[2] && ids->ne[0] % b->ne[1] == 0);
    MI_ASSERT(dst->type == GGML_TYPE_F32 && dst->nb[0] == sizeof(float) && dst->ne[0] == as->ne[1] && dst->ne[1] == ids->ne[0] &&
              dst->ne[2] == b->ne[2]);
    const int64_t K = as->ne[0], N = as->ne[1], n_as = as->ne[2];
    const int64_t ne11 = b->ne[1], n_tokens = b->ne[2], n_ids = ids->ne[0];
    MI_ASSERT(n_as < INT32_MAX && n_ids * n_tokens < INT32_MAX);
    if (n_ids == 0 || n_tokens == 0 || N == 0) return;

    if (mmid_stream_eligible(dst)) {
        mi_mmv_group g;
        mmv_group_for(g, as, b->nb[1], 1, dst->nb[1]);
        g.n = (int) (n_ids * n_tokens);
        g.ids_w = as->data;
        g.ids_nb02 = as->nb[2];
        g.ids_n_as = (int) n_as;
        for (int64_t t = 0; t < n_tokens; t++) {
            for (int64_t e = 0; e < n_ids; e++) {
                mi_mmv_member & m = g.m[e + n_ids * t];
                m.W = (const char *) ids->data + e * ids->nb[0] + t * ids->nb[1];  // the id's address: resolved by the kernel
                m.X = (const char *) b->data + (e % ne11) * b->nb[1] + t * b->nb[2];
                m.dst = (float *) ((char *) dst->data + e * dst->nb[1] + t * dst->nb[2]);
            }
        }
        mi_mul_mat_q_fused(g, ctx->stream);
        ctx->last_launches++;
        return;
    }

    mi_mm_desc m = mm_desc(as, as->data, N, b, (float *) dst->data, dst->nb[1], dst->nb[2], dst->nb[3]);  // (ne03 = ne13 = 1: asserted above)
    m.id.ids = (const int32_t *) ids->data;
    m.id.nb0 = ids->nb[0];
    m.id.nb1 = ids->nb[1];
    m.id.n_as = (int) n_as;
    m.id.n_ids = (int) n_ids;

    const mi_act_format f = act_format_of(as->type);
    const int cap = g_mi_tuning.mmid_group == 8 ? 8 : 4;  // (chunks of 4 measured faster than 8 at every size, both orders)
    const bool grouped = f.layout == MI_LAYOUT_SOA && f.quant != MI_ACT_NONE && g_mi_tuning.mmid_group && n_as <= kMiMmidMaxExperts &&
                         n_tokens >= (g_mi_tuning.mmid_group > 1 ? 2 : mmid_group_min_tokens());
    // blockIdx.y counts the pairs, or the chunks of up to `cap` pairs
    MI_ASSERT((grouped ? mi_mmid_max_chunks(n_as, n_ids * n_tokens, cap) : n_ids * n_tokens) <= 65535 && "MUL_MAT_ID: too many pairs for one launch");
    if (f.quant == MI_ACT_NONE) {
        MI_ASSERT(as->type == GGML_TYPE_F32);
        mi_mul_mat_f32(m, src_cols(b), ctx->stream);
    } else {
        void * xa = get_activations(ctx, b, f, K);
        if (f.quant == MI_ACT_F16) {
            mi_mul_mat_f16(m, (const uint16_t *) xa, ctx->stream);
        } else if (f.quant == MI_ACT_BF16) {
            mi_mul_mat_bf16(m, (const uint16_t *) xa, ctx->stream);
        } else {
            if (grouped) {
                const int64_t pairs = n_ids * n_tokens;
                m.id.chunk_cap = cap;
                int4 * chunks = (int4 *) scratch_take(ctx, (size_t) mi_mmid_max_chunks(n_as, pairs, cap) * sizeof(int4));
                int32_t * plist = (int32_t *) scratch_take(ctx, (size_t) pairs * sizeof(int32_t));
                mi_mmid_group(m.id, n_tokens, chunks, plist, ctx->stream);
                ctx->last_launches++;
                m.id.chunks = chunks;
                m.id.pairs = plist;
            }
            mi_mul_mat_q(m, mi_act_q8_carve(xa, K, ne11 * n_tokens, f.quant), ctx->stream);
        }
    }
    ctx->last_launches++;
}

// Per-slot helper context of the split path: its own stream (on the slot's device), scratch and
// activation cache, plus the event that hands the slot's gathered rows back to the caller.
struct mi_split_aux {
    mi_backend_ctx ctx;
    hipEvent_t done = nullptr;
};

static mi_split_aux * split_aux(int slot, int main_device) {
    static std::mutex mutex;
    static mi_split_aux * aux[GGML_MI355X_MAX_DEVICES] = {};
    std::lock_guard<std::mutex> lock(mutex);
    if (!aux[slot]) {
        auto * a = new mi_split_aux();
        a->ctx.device = slot_device(slot);
        a->ctx.name = "MI355X_Split" + std::to_string(slot);
        mi_device_guard g(a->ctx.device);
        MI_CHECK(hipStreamCreateWithFlags(&a->ctx.stream, hipStreamNonBlocking));
        MI_CHECK(hipEventCreateWithFlags(&a->done, hipEventDisableTiming));
        aux[slot] = a;
    }
    if (aux[slot]->ctx.device != main_device) {
        // peer access both ways for the activation copy in and the row gather out (xGMI)
        for (const auto & pr : {std::make_pair(aux[slot]->ctx.device, main_device), std::make_pair(main_device, aux[slot]->ctx.device)}) {
            mi_device_guard g(pr.first);
            const hipError_t e = hipDeviceEnablePeerAccess(pr.second, 0);
            if (e != hipSuccess) (void) hipGetLastError();  // already enabled
        }
    }
    return aux[slot];
}

// GGML_OP_MUL_MAT with a weight in the split buffer type (ggml-cuda.cu:1360-1647 analogue): the
// slot on the backend's own device computes its rows in place into dst; every other slot gets the
// activations copied to its device (peer copy over xGMI), computes its rows on its own stream into
// local scratch, and copies them back into dst's row range (a pitched copy), ordered by events.
// As the reference quantizes src1 once and ships the q8_1 blocks (ggml-cuda.cu:1551-1565), the
// activations are converted ONCE on the main device, in the format the slots' kernels read (q8_K
// / q8_0 blocks, or f16), and those bytes travel -- for Q4_K at K = 4096 4.4 KB per column
// instead of the f32 column's 16 KB; only F32 weights ship f32.
void op_mul_mat_split(mi_backend_ctx * ctx, ggml_tensor * dst) {
    const ggml_tensor * src0 = dst->src[0];
    const ggml_tensor * src1 = dst->src[1];
    MI_ASSERT(src0->view_src == nullptr && "views of split tensors are not supported");
    MI_ASSERT(src0->ne[2] == 1 && src0->ne[3] == 1 && src1->ne[2] == 1 && src1->ne[3] == 1);
    MI_ASSERT(src1->type == GGML_TYPE_F32 && ggml_is_contiguous(src1) && dst->nb[0] == sizeof(float));
    const auto * extra = (const mi_split_extra *) src0->extra;
    const int64_t K = src0->ne[0], ncols = src1->ne[1];
    // the backend's own slot (the first slot placed on its device) runs in place; further slots on
    // the same device (GGML_MI355X_SPLIT_SLOTS > device count) take the copy path
    auto is_local = [&](const mi_split_slice & sl) { return sl.device == ctx->device && sl.slot == ctx->device % split_slots(); };
    // the activation format of each remote slot's mul_mat, converted on the main stream first
    struct remote {
        const mi_split_slice * sl;
        int64_t ld;
        mi_act_format xf; // the format shipped (quant MI_ACT_NONE: the f32 columns)
        const void * xa;  // converted activations on the main device
    };
    std::vector<remote> rem;
    for (const auto & sl : extra->slices) {
        if (is_local(sl)) continue;
        const int64_t rows = sl.row_high - sl.row_low;
        remote rm{&sl, (rows + 3) & ~(int64_t) 3, {}, src1->data};
        const size_t ycol = (size_t) rm.ld * sizeof(float);
        rm.xf = mm_act_format(mm_desc(src0, sl.ptr, rows, src1, nullptr, ycol, ycol * ncols, ycol * ncols), src1);
        if (rm.xf.quant != MI_ACT_NONE) rm.xa = get_activations(ctx, src1, rm.xf, K);
        rem.push_back(rm);
    }
    if (!rem.empty()) {
        mi_device_guard g(ctx->device);
        if (!ctx->split_ready) MI_CHECK(hipEventCreateWithFlags(&ctx->split_ready, hipEventDisableTiming));
        MI_CHECK(hipEventRecord(ctx->split_ready, ctx->stream));  // src1 and its conversions are ready
    }
    for (const auto & sl : extra->slices) {
        if (!is_local(sl)) continue;
        mul_mat_run(ctx, src0, sl.ptr, sl.row_high - sl.row_low, src1, (float *) ((char *) dst->data + sl.row_low * sizeof(float)),
                    dst->nb[1], dst->nb[2], dst->nb[3]);
    }
    std::vector<mi_split_aux *> waits;
    for (const remote & rm : rem) {
        const mi_split_slice & sl = *rm.sl;
        const int64_t rows = sl.row_high - sl.row_low;
        float * out = (float *) ((char *) dst->data + sl.row_low * sizeof(float));
        mi_split_aux * a = split_aux(sl.slot, ctx->device);
        mi_device_guard g(a->ctx.device);
        MI_CHECK(hipStreamWaitEvent(a->ctx.stream, ctx->split_ready, 0));
        const size_t xbytes = rm.xf.quant != MI_ACT_NONE ? act_bytes(rm.xf, K, ncols) : (size_t) K * ncols * sizeof(float);
        const size_t ybytes = (size_t) rm.ld * ncols * sizeof(float);
        scratch_reserve(&a->ctx, xbytes + ybytes + 4 * kBufferAlign);  // stream-ordered reuse: earlier users ran on the same stream
        a->ctx.scratch_used = 0;
        a->ctx.act_cache.clear();
        void * xl = scratch_take(&a->ctx, xbytes);
        float * yl = (float *) scratch_take(&a->ctx, ybytes);
        if (a->ctx.device == ctx->device) {
            MI_CHECK(hipMemcpyAsync(xl, rm.xa, xbytes, hipMemcpyDeviceToDevice, a->ctx.stream));
        } else {
            MI_CHECK(hipMemcpyPeerAsync(xl, a->ctx.device, rm.xa, ctx->device, xbytes, a->ctx.stream));
        }
        ggml_tensor x1 = *src1;  // src1 as the slot sees it (the f32 columns or their conversion)
        x1.data = xl;
        x1.view_src = nullptr;
        x1.view_offs = 0;
        // the slot's mul_mat finds its activations already converted
        if (rm.xf.quant != MI_ACT_NONE) cache_activations(&a->ctx, &x1, rm.xf, xl);
        a->ctx.last_launches = 0;
        mul_mat_run(&a->ctx, src0, sl.ptr, rows, &x1, yl, (size_t) rm.ld * sizeof(float), (size_t) rm.ld * ncols * sizeof(float),
                    (size_t) rm.ld * ncols * sizeof(float));
        ctx->last_launches += a->ctx.last_launches;
        MI_CHECK(hipMemcpy2DAsync(out, dst->nb[1], yl, (size_t) rm.ld * sizeof(float), (size_t) rows * sizeof(float), (size_t) ncols,
                                  hipMemcpyDeviceToDevice, a->ctx.stream));
        MI_CHECK(hipEventRecord(a->done, a->ctx.stream));
        waits.push_back(a);
    }
    mi_device_guard g(ctx->device);
    for (mi_split_aux * a : waits) MI_CHECK(hipStreamWaitEvent(ctx->stream, a->done, 0));
}

// ---- launches that serve several nodes: independent mul_mats in one grid -------------------

// n items over launches of at most cap each, split evenly (36 -> 18 + 18, not 32 + 4: a launch of few
// members is all prologue): the share of each launch but the last
static int64_t even_share(int64_t n, int64_t cap) {
    const int64_t launches = (n + cap - 1) / cap;
    return (n + launches - 1) / launches;
}

// The members of the grouped launch that starts at nodes[i], as node indices: nodes[i], then the
// nodes that follow (`next` steps from one candidate to the next, -1 at the end) while `belongs`
// holds and the node is independent of every member before it -- neither reads what one writes nor
// writes what one reads or writes. Up to 4 launches' worth is scanned; the first even share is returned.
template <class Next, class Belongs>
static std::vector<int> collect_run(const ggml_cgraph * g, int i, int cap, Next next, Belongs belongs) {
    std::vector<int> at = {i};
    for (int j = next(i); j >= 0 && (int) at.size() < 4 * cap; j = next(j)) {
        const ggml_tensor * n = g->nodes[j];
        if (!belongs(n)) break;
        bool independent = true;
        for (int k : at) {
            const ggml_tensor * m = g->nodes[k];
            if (overlaps(n->src[1], m) || overlaps(n->src[0], m) || overlaps(n, m->src[0]) || overlaps(n, m->src[1]) || overlaps(n, m)) {
                independent = false;
                break;
            }
        }
        if (!independent) break;
        at.push_back(j);
    }
    at.resize((size_t) even_share((int64_t) at.size(), cap));
    return at;
}

// Decode: launches nodes[i] and following independent same-shape mul_mats as one streaming GEMV that
// quantizes the activations itself. Returns the index of the last node consumed.
static int run_fused_group(mi_backend_ctx * ctx, ggml_cgraph * cgraph, int i) {
    static_assert(sizeof(mi_mmv_group) < 4096, "kernel argument block");
    const ggml_tensor * first = cgraph->nodes[i];
    // (only no-ops are stepped over: an absorbed node in between ends the run)
    auto next = [&](int j) {
        for (j++; j < cgraph->n_nodes; j++) {
            if (!is_noop(cgraph->nodes[j])) return j;
        }
        return -1;
    };
    const std::vector<int> at = collect_run(cgraph, i, kMiMaxMembers, next,
                                            [&](const ggml_tensor * n) { return fused_mv_eligible(n) && same_group_shape(first, n); });
    mi_mmv_group g;
    mmv_group_for(g, first->src[0], first->src[1]->nb[1], (int) first->src[1]->ne[1], first->nb[1]);
    g.n = (int) at.size();
    const ggml_tensor * wts[kMiMaxMembers];
    for (int m = 0; m < g.n; m++) {
        const ggml_tensor * n = cgraph->nodes[at[m]];
        g.m[m].W = n->src[0]->data;
        g.m[m].X = (const char *) n->src[1]->data;
        g.m[m].dst = (float *) n->data;
        wts[m] = n->src[0];
    }
    q40r_apply(ctx, g, wts);
    mi_mul_mat_q_fused(g, ctx->stream);
    ctx->last_launches++;
    for (int k : at) invalidate_activations(ctx, cgraph->nodes[k]);
    return at.back();
}

// Quantized prompt mul_mats in a reference-order graph (mmv_order 1, or -1 resolved to 1: a quantized
// model's graph): the int8-MFMA prefill GEMMs compute the reference's exact integer block sums but
// fold them in their own canonical order, and since every layer re-quantizes its activations an ulp
// there becomes a quant step (~1e-2 of max|logit|). Such a mul_mat -- any column count since round 6
// -- runs instead as the reference-order streaming GEMV (k_mmv_stream ORD: the CPU's vec_dot lane
// chains, bit-identical; ggml.c:12056-12096 runs every column through the same vec_dot) over
// 8-column chunks, up to kMiMaxMembers chunks per launch: each chunk is a member of one grouped
// launch over the same weight rows, so a 512-column prompt is one launch whose chunks re-read the
// weights from the caches rather than 64 dependent launches. The knob ord_prefill_cols caps the
// column count (longer prompts take the MFMA GEMMs), 0 turns it off; in tree order prompts of up to
// tree_prefill_cols columns take the same 8-column GEMV chunks.
static bool ord_prefill_chunked(const ggml_tensor * n) {
    if (n->op != GGML_OP_MUL_MAT || is_split_tensor(n->src[0])) return false;
    const ggml_tensor * a = n->src[0];
    const ggml_tensor * b = n->src[1];
    if (b->type != GGML_TYPE_F32 || b->ne[1] <= 8 || b->ne[1] > (mi_mmv_order() == 1 ? g_mi_tuning.ord_prefill_cols : g_mi_tuning.tree_prefill_cols)) return false;
    if (!mi_mmv_fused_supported(a->type, a->ne[0], 8)) return false;
    if (!plain_2d_operands(n) || !fused_weight_aligned(a) || !f32_cols_aligned(b)) return false;
    // beyond fused_mv_eligible: each chunk's output starts a whole number of columns into dst, and no
    // epilogue pass has checked that dst lies clear of the operands
    return n->nb[1] % sizeof(float) == 0 && !overlaps(n, a) && !overlaps(n, b);
}

static void run_ord_prefill_chunks(mi_backend_ctx * ctx, ggml_tensor * n) {
    const ggml_tensor * a = n->src[0];
    const ggml_tensor * b = n->src[1];
    const int64_t ncols = b->ne[1];
    const int64_t full = ncols / 8;  // 8-column chunks; the ragged tail (< 8 columns) is one more launch
    auto launch = [&](int64_t c_first, int64_t nchunks, int cols) {
        mi_mmv_group g;
        mmv_group_for(g, a, b->nb[1], cols, n->nb[1]);
        g.n = (int) nchunks;
        for (int64_t k = 0; k < nchunks; k++) {
            const int64_t c0 = c_first + 8 * k;
            g.m[k].W = a->data;
            g.m[k].X = (const char *) b->data + c0 * b->nb[1];
            g.m[k].dst = (float *) ((char *) n->data + c0 * n->nb[1]);
        }
        mi_mul_mat_q_fused(g, ctx->stream);
        ctx->last_launches++;
    };
    if (full > 0) {
        const int64_t take = even_share(full, kMiMaxMembers);
        for (int64_t k0 = 0; k0 < full; k0 += take) launch(8 * k0, std::min<int64_t>(take, full - k0), 8);
    }
    if (ncols % 8) launch(8 * full, 1, (int) (ncols % 8));
}

// the activation format of a MUL_MAT node that runs on an exact int8 prefill GEMM (q8_K or q8_0
// in the MFMA layout; > 8 plain columns), or none (quant MI_ACT_NONE)
static mi_act_format prefill_mmx_format(const ggml_tensor * n) {
    if (n->op != GGML_OP_MUL_MAT || is_split_tensor(n->src[0]) || ord_prefill_chunked(n)) return {};
    const ggml_tensor * a = n->src[0], * b = n->src[1];
    // (no alignment asked here: mm_batched and the GEMM's own mi_mmqx_supported decide, below; mm_batched
    // refuses operands that are not 2-D as well)
    if (b->type != GGML_TYPE_F32 || !plain_2d_operands(n) || a->ne[0] != b->ne[0]) return {};
    const mi_act_format f = mm_act_format(mm_desc_of(n), b);
    return f.layout == MI_LAYOUT_MFMA ? f : mi_act_format{};
}

// Batched (prompt) mul_mats that follow each other in the graph and are independent of each other
// (Q/K/V or gate/up projections of one prompt, independent prompts), same weight type, K and
// column count: their activations are quantized by ONE launch (each distinct src1 once) and their
// GEMMs run as ONE grouped launch (mi_mul_mat_mmqx_group: every member's tiles in one grid), so
// a short prompt pays two kernel boundaries per group instead of per mul_mat. Each member's
// output is what op_mul_mat computes for it, bit for bit (same kernels, same fold). Returns the
// index of the last node consumed, or -1 (fewer than two members).
static int run_prefill_group(mi_backend_ctx * ctx, ggml_cgraph * g, int i) {
    const ggml_tensor * first = g->nodes[i];
    const mi_act_format f = prefill_mmx_format(first);
    if (mi_env().no_prefill_group || f.quant == MI_ACT_NONE) return -1;
    const ggml_type type = first->src[0]->type;
    const int64_t K = first->src[0]->ne[0];
    auto cols_of = [](const ggml_tensor * n) { return n->src[1]->ne[1] * n->src[1]->ne[2] * n->src[1]->ne[3]; };
    const int64_t ncols = cols_of(first);
    // (next_node steps over absorbed nodes too, unlike run_fused_group)
    const std::vector<int> at = collect_run(g, i, kMiMaxPrefillMembers, [&](int j) { return next_node(g, j); }, [&](const ggml_tensor * n) {
        return prefill_mmx_format(n) == f && n->src[0]->type == type && n->src[0]->ne[0] == K && cols_of(n) == ncols;
    });
    if (at.size() < 2) return -1;
    // activations: cached conversions are reused; the missing distinct src1s in one quantizer launch
    mi_mmx_qgroup q;
    q.K = K;
    std::vector<void *> xa(at.size(), nullptr);
    for (size_t k = 0; k < at.size(); k++) {
        const ggml_tensor * x = g->nodes[at[k]]->src[1];
        xa[k] = find_activations(ctx, x, f);
        if (xa[k]) continue;
        void * dev = scratch_take(ctx, act_bytes(f, K, ncols));
        q.m[q.n].x = src_cols(x);
        q.m[q.n].act = mmx_carve(f.quant, dev, K, ncols);
        q.n++;
        cache_activations(ctx, x, f, dev);
        xa[k] = dev;
    }
    if (q.n > 0) {
        if (f.quant == MI_ACT_Q8_K) mi_quantize_q8_K_mmx_group(q, ctx->stream);
        else mi_quantize_q8_0_mmx_group(q, ctx->stream);
        ctx->last_launches++;
    }
    mi_mmx_group gg;
    gg.type = type;
    gg.K = K;
    gg.n = (int) at.size();
    for (size_t k = 0; k < at.size(); k++) {
        const ggml_tensor * n = g->nodes[at[k]];
        const mi_act_mmx act = mmx_carve(f.quant, xa[k], K, ncols);
        gg.m[k] = mi_mmx_member{n->src[0]->data, n->src[0]->nb[1], n->src[0]->ne[1], act, (float *) n->data, n->nb[1], 0, planes_of(ctx, n->src[0], n->src[1])};
    }
    mi_mul_mat_mmqx_group(gg, ctx->stream);
    ctx->last_launches++;
    for (int k : at) invalidate_activations(ctx, g->nodes[k]);
    return at.back();
}

// A MUL_MAT node that no fusion pass took (its weight not split): the decode group, the chunked
// prompt, the prompt group, or the node on its own. Returns the last node consumed; the outputs of
// all of them are invalidated.
int run_mul_mat(mi_backend_ctx * ctx, ggml_cgraph * g, int i) {
    ggml_tensor * node = g->nodes[i];
    if (!mi_env().no_fused_mmv && fused_mv_eligible(node)) return run_fused_group(ctx, g, i);
    if (ord_prefill_chunked(node)) {
        run_ord_prefill_chunks(ctx, node);
    } else {
        const int last = run_prefill_group(ctx, g, i);
        if (last >= 0) return last;
        op_mul_mat(ctx, node);
    }
    invalidate_activations(ctx, node);
    return i;
}
