// ops.cpp -- what the MI355X backend supports and offloads (src/ggml-cuda.cu:2715-2868 analogue), and
// the dispatch of every op that is no mul_mat into the kernels of csrc/kernels/ (:2156-2308
// analogue): the companion ops with their fp16 and RoPE tables, and FLASH_ATTN_EXT.

#include "mi_backend.h"

// ---------------------------------------------------------------------------------------------
// op support (ggml-cuda.cu:2715-2859 analogue; the scheduler does not consult it, the
// conformance harness does)
// ---------------------------------------------------------------------------------------------

// IQ4_NL rows of an odd block count: the reference's AVX2 ggml_vec_dot_iq4_nl_q8_0 walks the blocks in
// pairs with no tail and reads past the row, so it defines no result to agree with
static bool mm_row_supported(const ggml_tensor * a) { return a->type != GGML_TYPE_IQ4_NL || a->ne[0] % 64 == 0; }

// the dense element types CPY / DUP / CONT convert between (the element-wise ops take F32 / F16 only)
static bool is_dense(const ggml_tensor * t) { return is_f16_or_f32(t) || (t && t->type == GGML_TYPE_BF16); }

bool mi_supports_op(ggml_backend_t, const ggml_tensor * op) {
    const ggml_tensor * a = op->src[0];
    const ggml_tensor * b = op->src[1];
    switch (op->op) {
        case GGML_OP_NONE:
        case GGML_OP_RESHAPE:
        case GGML_OP_VIEW:
        case GGML_OP_PERMUTE:
        case GGML_OP_TRANSPOSE:
            return true;
        case GGML_OP_MUL_MAT: {
            if (!mm_src0_supported(a->type) || !mm_row_supported(a)) return false;
            if (a->nb[0] != ggml_type_size(a->type) || b->nb[0] != ggml_type_size(b->type)) return false;
            // src1 F32, or src1 already of the weight's vec_dot_type, which the reference CPU reads as
            // it lies (ggml.c:11952; F16 x F16, BF16 x BF16, Q4_K/Q5_K/Q6_K x Q8_K, Q4_0/Q5_0/Q8_0 x Q8_0, Q4_1/Q5_1 x Q8_1): the quantized
            // ones with whole superblocks, on the device's own weights
            // (the split-buffer path converts an F32 src1 on the main device: F16 / BF16 src1 only unsplit)
            if (b->type == GGML_TYPE_F32 || ((b->type == GGML_TYPE_F16 || b->type == GGML_TYPE_BF16) && a->type == b->type && !is_split_tensor(a))) return true;
            return b->type == q8_src1_type(a->type) && a->ne[0] % 256 == 0 && !is_split_tensor(a);
        }
        case GGML_OP_MUL_MAT_ID: {
            // experts of any mul_mat weight type on this device, F32 activations (quantized or converted
            // here, as the reference does), I32 ids read by the kernels
            const ggml_tensor * ids = op->src[2];
            if (!mm_src0_supported(a->type) || !mm_row_supported(a) || is_split_tensor(a)) return false;
            if (a->nb[0] != ggml_type_size(a->type) || b->nb[0] != ggml_type_size(b->type)) return false;
            return b->type == GGML_TYPE_F32 && ids && ids->type == GGML_TYPE_I32;
        }
        case GGML_OP_FLASH_ATTN_EXT: {
            // F32 q, an F16 K/V cache (any row / head / batch strides) of a head size the kernels are
            // built for, heads that divide, a contiguous F16 mask padded as the builder asks, or none
            const ggml_tensor * v = op->src[2];
            const ggml_tensor * mask = op->src[3];
            if (!is_f32(a) || a->nb[0] != sizeof(float) || !is_f32(op) || !ggml_is_contiguous(op)) return false;
            if (!b || !v || b->type != GGML_TYPE_F16 || v->type != GGML_TYPE_F16 || b->nb[0] != 2 || v->nb[0] != 2) return false;
            if (!mi_fa_head_size_ok(b->ne[0]) || a->ne[0] != b->ne[0] || v->ne[0] != b->ne[0] || v->ne[1] != b->ne[1]) return false;
            if (b->ne[1] < 1 || a->ne[1] < 1) return false;
            if (a->ne[2] % b->ne[2] != 0 || a->ne[2] % v->ne[2] != 0 || a->ne[3] % b->ne[3] != 0 || a->ne[3] % v->ne[3] != 0) return false;
            if (mask && (mask->type != GGML_TYPE_F16 || !ggml_is_contiguous(mask) || mask->ne[0] < b->ne[1] ||
                         mask->ne[1] < GGML_PAD(a->ne[1], GGML_KQ_MASK_PAD)))
                return false;
            if (op_param_f(op, 1) > 0.0f && !mask) return false;
            return !is_split_tensor(a) && !is_split_tensor(b) && !is_split_tensor(v) && !(mask && is_split_tensor(mask));
        }
        case GGML_OP_SSM_CONV: {
            // F32 state / x / weights and an I32 sq the kernel reads, with the strides the reference forward
            // asserts (src/ggml.c:16331-16338): contiguous state rows, contiguous weights, x rows of any stride
            const ggml_tensor * c = op->src[2];
            const ggml_tensor * sq = op->src[3];
            if (!a || !b || !c || !sq || !is_f32(a) || !is_f32(b) || !is_f32(c) || !is_f32(op) || sq->type != GGML_TYPE_I32) return false;
            if (!mi_ssm_conv_width_ok(c->ne[0]) || !ggml_is_3d(a) || !ggml_is_matrix(b) || !ggml_is_matrix(c) || !ggml_is_matrix(sq)) return false;
            if (a->ne[0] != c->ne[0] - 1 || a->ne[1] != c->ne[1] || b->ne[0] != c->ne[1] || sq->ne[0] != a->ne[2] || sq->ne[1] != b->ne[1]) return false;
            if (a->nb[0] != sizeof(float) || a->nb[1] != (size_t) a->ne[0] * sizeof(float) || b->nb[0] != sizeof(float) ||
                !ggml_is_contiguous(c) || sq->nb[0] != sizeof(int32_t) || !ggml_is_contiguous(op))
                return false;
            if (ggml_nelements(op) != b->ne[0] * b->ne[1] + c->ne[0] * c->ne[1] * a->ne[2]) return false;
            return !is_split_tensor(a) && !is_split_tensor(b) && !is_split_tensor(c) && !is_split_tensor(sq);
        }
        case GGML_OP_SSM_SCAN: {
            // F32 everywhere and an I32 sq; the strides of src/ggml.c:16460-16472: contiguous s and x, unit
            // element stride in dt / A / B / C (B and C are views of wider rows in a model graph)
            for (int i = 0; i < 7; i++) {
                const ggml_tensor * t = op->src[i];
                if (!t || t->type != (i == 6 ? GGML_TYPE_I32 : GGML_TYPE_F32) || t->nb[0] != 4 || is_split_tensor(t)) return false;
            }
            const ggml_tensor * dt = op->src[2], * A = op->src[3], * B = op->src[4], * C = op->src[5], * sq = op->src[6];
            if (!is_f32(op) || !ggml_is_contiguous(op) || !ggml_is_contiguous(a) || !ggml_is_contiguous(b) || !ggml_is_3d(a)) return false;
            if (!ggml_is_matrix(b) || !ggml_is_matrix(dt) || !ggml_is_matrix(A) || !ggml_is_matrix(B) || !ggml_is_matrix(C) || !ggml_is_matrix(sq)) return false;
            const int64_t d_state = a->ne[0], d_inner = a->ne[1], n_t = b->ne[1];
            if (d_state < 1 || b->ne[0] != d_inner || !ggml_are_same_shape(b, dt) || A->ne[0] != d_state || A->ne[1] != d_inner) return false;
            if (B->ne[0] != d_state || B->ne[1] != n_t || C->ne[0] != d_state || C->ne[1] != n_t || sq->ne[0] != a->ne[2] || sq->ne[1] != n_t) return false;
            return ggml_nelements(op) == ggml_nelements(b) + ggml_nelements(a);
        }
        case GGML_OP_ADD:
        case GGML_OP_SUB:
        case GGML_OP_MUL:
        case GGML_OP_DIV:
            return is_f16_or_f32(a) && is_f16_or_f32(b) && is_f16_or_f32(op);
        case GGML_OP_SCALE:
            return is_f32(a) && is_f32(op);
        case GGML_OP_SUM_ROWS:
            return is_f32(a) && is_f32(op) && a->nb[0] == sizeof(float) && op->nb[0] == sizeof(float);
        case GGML_OP_ARGSORT:
            // f32 rows that one workgroup holds a position per thread (router.hip)
            return is_f32(a) && op->type == GGML_TYPE_I32 && a->nb[0] == sizeof(float) && op->nb[0] == sizeof(int32_t) &&
                   a->ne[0] <= kMiArgsortMaxRow;
        case GGML_OP_NORM:
        case GGML_OP_RMS_NORM:
            // rows longer than the kernel's LDS staging (12288 floats) stage in a contiguous dst
            return is_f32(a) && is_f32(op) && a->nb[0] == sizeof(float) && (a->ne[0] <= 12288 || ggml_is_contiguous(op));
        case GGML_OP_SOFT_MAX: {
            float max_bias;
            memcpy(&max_bias, (const float *) op->op_params + 1, sizeof(float));
            return is_f32(a) && is_f32(op) && max_bias == 0.0f && (!b || is_f16_or_f32(b)) && ggml_is_contiguous(a);
        }
        case GGML_OP_DIAG_MASK_INF:
        case GGML_OP_DIAG_MASK_ZERO:
            return is_f32(a) && is_f32(op);
        case GGML_OP_UNARY:
            switch (ggml_get_unary_op(op)) {
                case GGML_UNARY_OP_GELU:
                case GGML_UNARY_OP_SILU:
                    return is_f32(a) && is_f32(op);
                default:
                    return false;
            }
        case GGML_OP_GET_ROWS:
            return mi_type(a->type).get_rows && b->type == GGML_TYPE_I32 && is_f32(op);
        case GGML_OP_CPY:
        case GGML_OP_DUP:
        case GGML_OP_CONT:
            // F32 -> Q8_K / Q8_0 / Q8_1 (from_float = quantize_row_q8_K / _q8_0 / _q8_1): whole rows of blocks
            if (is_f32(a) && q8_quant_of(op->type) != MI_ACT_NONE)
                return ggml_are_same_shape(a, op) && a->nb[0] == sizeof(float) && op->nb[0] == ggml_type_size(op->type) &&
                       op->ne[0] % mi_act_block(q8_quant_of(op->type)) == 0;
            // F32 / F16 / BF16 in any pairing (to BF16: ggml_fp32_to_bf16's bits, F16 through f32)
            return is_dense(a) && is_dense(op);
        case GGML_OP_ROPE: {
            const int32_t * pp = (const int32_t *) op->op_params;
            const int mode = pp[2];
            float xpos_base;
            memcpy(&xpos_base, pp + 11, sizeof(float));
            return is_f32(a) && is_f32(op) && (mode == 0 || mode == 2) && xpos_base == 0.0f && a->nb[0] == sizeof(float);
        }
        default:
            return false;
    }
}

bool mi_offload_op(ggml_backend_t, const ggml_tensor * op) {
    // worth moving CPU-resident weights for batched work (ggml-cuda.cu:2861-2868 uses 32)
    return op->ne[1] >= 32 && op->op != GGML_OP_GET_ROWS;
}

// ---------------------------------------------------------------------------------------------
// companion ops (GPT-2 / LLaMA-shaped graphs)
// ---------------------------------------------------------------------------------------------

static uint16_t host_f2h(float f) {  // round-to-nearest-even, as F16C _cvtss_sh(x, 0)
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t ax = x & 0x7fffffffu;
    if (ax > 0x7f800000u) return (uint16_t) (sign | 0x7e00u | ((ax >> 13) & 0x3ffu));
    if (ax >= 0x477ff000u) return (uint16_t) (sign | 0x7c00u);
    if (ax < 0x38800000u) {  // subnormal half
        const float v = fabsf(f) * 16777216.0f;  // exact scaling by 2^24
        return (uint16_t) (sign | (uint32_t) nearbyintf(v));
    }
    const uint32_t r = ax + 0xfffu + ((ax >> 13) & 1u) - 0x38000000u;
    return (uint16_t) (sign | (r >> 13));
}

static float host_h2f(uint16_t h) {
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ff;
    float r;
    if (e == 0) r = ldexpf((float) m, -24);
    else if (e == 31) r = m ? NAN : INFINITY;
    else r = ldexpf((float) (m | 0x400), (int) e - 25);
    uint32_t u;
    memcpy(&u, &r, 4);
    u |= sign;
    memcpy(&r, &u, 4);
    return r;
}

// the reference's fp16 lookup tables (src/ggml.c:2884-2898), same formulas and libm
static const float kGeluCoefA = 0.044715f;
static const float kSqrt2OverPi = 0.79788456080286535587989211986876f;
// ggml_gelu_f32 as the reference's gcc -O3 -mfma build evaluates it (read off its ggml_init):
// (0.5f*x) * (1 + tanhf((SQRT_2_OVER_PI*x) * fmaf(GELU_COEF_A*x, x, 1))) -- one contraction
static float gelu_ref(float x) {
    const float inner = fmaf(kGeluCoefA * x, x, 1.0f);
    const float arg = (kSqrt2OverPi * x) * inner;
    return (0.5f * x) * (1.0f + tanhf(arg));
}
static float silu_ref(float x) { return x / (1.0f + expf(-x)); }

const uint16_t * op_tables(mi_backend_ctx * ctx) {
    if (!ctx->tables) {
        std::vector<uint16_t> h(3 * 65536);
        for (int i = 0; i < 65536; i++) {
            const float f = host_h2f((uint16_t) i);
            h[i] = host_f2h(expf(f));
            h[65536 + i] = host_f2h(gelu_ref(f));
            h[2 * 65536 + i] = host_f2h(silu_ref(f));
        }
        MI_CHECK(hipMalloc(&ctx->tables, h.size() * sizeof(uint16_t)));
        MI_CHECK(hipMemcpy(ctx->tables, h.data(), h.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    return ctx->tables;
}

mi_tensor_desc desc(const ggml_tensor * t) {
    mi_tensor_desc d;
    d.data = t ? (char *) t->data : nullptr;
    d.type = t ? (int) t->type : 0;
    for (int i = 0; i < 4; i++) {
        d.ne[i] = t ? t->ne[i] : 1;
        d.nb[i] = t ? t->nb[i] : 0;
    }
    return d;
}


// ggml_rope_yarn_corr_dims (src/ggml.c:13746-13773)
static void rope_corr_dims(int n_dims, int n_orig_ctx, float freq_base, float beta_fast, float beta_slow, float dims[2]) {
    auto corr_dim = [&](float n_rot) {
        return n_dims * logf(n_orig_ctx / (n_rot * 2 * (float) M_PI)) / (2 * logf(freq_base));
    };
    const float start = floorf(corr_dim(beta_fast));
    const float end = ceilf(corr_dim(beta_slow));
    dims[0] = std::max(0.0f, start);
    dims[1] = std::min((float) (n_dims - 1), end);
}

// ---- RoPE {cos, sin} tables, built on the host exactly as the reference CPU computes them ----
// ggml_rope_cache_init / the NeoX loop of ggml_compute_forward_rope_f32 (src/ggml.c:13719-13948)
// and rope_yarn (:13680-13700) over positions 0 .. P-1, with the host libm's sincosf (the function
// the reference build calls) and the contractions its -mfma build makes (read off the object:
// theta = fma(theta_interp, 1 - ramp_mix, theta_extrap * ramp_mix); mscale *= fma(logf(1 /
// freq_scale), 0.1f, 1.0f)). Device positions outside [0, P) fall back to the kernel's own math.
#pragma clang fp contract(off)
static void rope_yarn_host(float theta_extrap, float freq_scale, const float corr[2], int64_t i0, float ext_factor, float mscale,
                           float * c, float * s) {
    const float theta_interp = freq_scale * theta_extrap;
    float theta = theta_interp;
    if (ext_factor != 0.0f) {
        const float y = ((float) (i0 / 2) - corr[0]) / std::max(0.001f, corr[1] - corr[0]);
        const float ramp_mix = (1.0f - std::min(1.0f, std::max(0.0f, y))) * ext_factor;
        theta = std::fma(theta_interp, 1.0f - ramp_mix, theta_extrap * ramp_mix);
        mscale *= std::fma(logf(1.0f / freq_scale), 0.1f, 1.0f);
    }
    float sv, cv;
    sincosf(theta, &sv, &cv);
    *c = cv * mscale;
    *s = sv * mscale;
}

static const mi_backend_ctx::rope_table * rope_table_find(mi_backend_ctx * ctx, int n_dims, int ne0, int mode, float fb, float fs,
                                                          float ef, float af, const float corr[2]) {
    for (const auto & t : ctx->rope_tables) {
        if (t.n_dims == n_dims && t.ne0 == ne0 && t.mode == mode && t.freq_base == fb && t.freq_scale == fs && t.ext_factor == ef &&
            t.attn_factor == af && t.corr0 == corr[0] && t.corr1 == corr[1]) return &t;
    }
    return nullptr;
}

// builds the table of a ROPE node if missing (synchronous upload: never while capturing)
void rope_table_ensure(mi_backend_ctx * ctx, const ggml_tensor * node) {
    const int32_t * pp = (const int32_t *) node->op_params;
    const int n_dims = pp[1], mode = pp[2], n_ctx = pp[3], n_orig_ctx = pp[4];
    const float fb = op_param_f(node, 5), fs = op_param_f(node, 6), ef = op_param_f(node, 7), af = op_param_f(node, 8);
    float corr[2];
    rope_corr_dims(n_dims, n_orig_ctx, fb, op_param_f(node, 9), op_param_f(node, 10), corr);
    const int ne0 = (int) node->src[0]->ne[0];
    if ((mode != 0 && mode != 2) || n_dims <= 0 || n_dims % 2 || rope_table_find(ctx, n_dims, ne0, mode, fb, fs, ef, af, corr)) return;
    const int P = std::min(std::max({n_ctx, n_orig_ctx, 4096}), 1 << 16);
    const int pairs = mode == 0 ? ne0 / 2 : n_dims / 2;
    std::vector<float> h((size_t) P * pairs * 2);
    const float theta_scale = powf(fb, -2.0f / n_dims);
    const float inv_ndims = -1.f / n_dims;
    for (int p = 0; p < P; p++) {
        float * row = h.data() + (size_t) p * pairs * 2;
        if (mode == 0) {
            float theta = (float) p;
            for (int k = 0; k < pairs; k++) {
                rope_yarn_host(theta, fs, corr, 2 * k, ef, af, &row[2 * k], &row[2 * k + 1]);
                theta *= theta_scale;
            }
        } else {
            float theta = (float) p;
            theta *= fs;
            for (int k = 0; k < pairs; k++) {
                const float cur_rot = inv_ndims * (float) (2 * k) - 0.0f;
                rope_yarn_host(theta, fs, corr, (int64_t) cur_rot, ef, af, &row[2 * k], &row[2 * k + 1]);
                theta *= theta_scale;
            }
        }
    }
    mi_backend_ctx::rope_table t{n_dims, ne0, mode, P, fb, fs, ef, af, corr[0], corr[1], nullptr};
    mi_device_guard g(ctx->device);
    MI_CHECK(hipMalloc(&t.dev, h.size() * sizeof(float)));
    MI_CHECK(hipMemcpy(t.dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->rope_tables.push_back(t);
}
#pragma clang fp contract(on)

void op_companion(mi_backend_ctx * ctx, ggml_tensor * node) {
    const ggml_tensor * a = node->src[0];
    const ggml_tensor * b = node->src[1];
    hipStream_t st = ctx->stream;
    switch (node->op) {
        case GGML_OP_ADD: mi_op_binary(desc(node), desc(a), desc(b), MI_OP_ADD, st); break;
        case GGML_OP_SUB: mi_op_binary(desc(node), desc(a), desc(b), MI_OP_SUB, st); break;
        case GGML_OP_MUL: mi_op_binary(desc(node), desc(a), desc(b), MI_OP_MUL, st); break;
        case GGML_OP_DIV: mi_op_binary(desc(node), desc(a), desc(b), MI_OP_DIV, st); break;
        case GGML_OP_SCALE: mi_op_unary(desc(node), desc(a), MI_OP_SCALE, op_param_f(node, 0), nullptr, st); break;
        case GGML_OP_NORM: mi_op_norm(desc(node), desc(a), op_param_f(node, 0), false, nullptr, nullptr, st); break;
        case GGML_OP_RMS_NORM: mi_op_norm(desc(node), desc(a), op_param_f(node, 0), true, nullptr, nullptr, st); break;
        case GGML_OP_SOFT_MAX: mi_op_soft_max(desc(node), desc(a), desc(b), op_param_f(node, 0), op_tables(ctx), 1.0f, -1, st); break;
        case GGML_OP_DIAG_MASK_INF:
            mi_op_diag_mask(desc(node), desc(a), ((const int32_t *) node->op_params)[0], -INFINITY, st);
            break;
        case GGML_OP_DIAG_MASK_ZERO:
            mi_op_diag_mask(desc(node), desc(a), ((const int32_t *) node->op_params)[0], 0.0f, st);
            break;
        case GGML_OP_UNARY: {
            const ggml_unary_op u = ggml_get_unary_op(node);
            MI_ASSERT(u == GGML_UNARY_OP_GELU || u == GGML_UNARY_OP_SILU);
            const uint16_t * t = op_tables(ctx) + (u == GGML_UNARY_OP_GELU ? 65536 : 2 * 65536);
            mi_op_unary(desc(node), desc(a), u == GGML_UNARY_OP_GELU ? MI_OP_GELU : MI_OP_SILU, 0.0f, t, st);
            break;
        }
        case GGML_OP_GET_ROWS: mi_op_get_rows(desc(node), desc(a), desc(b), st); break;
        case GGML_OP_SUM_ROWS: mi_op_sum_rows(desc(node), desc(a), st); break;
        case GGML_OP_ARGSORT:
            mi_op_argsort(desc(node), desc(a), ((const int32_t *) node->op_params)[0] == (int32_t) GGML_SORT_ORDER_DESC, st);
            break;
        case GGML_OP_SSM_CONV:
            // (ssm.hip) sq = src[3] is read by the kernel: a replayed capture follows new ids
            mi_op_ssm_conv(desc(node), desc(a), desc(b), desc(node->src[2]), desc(node->src[3]), st);
            break;
        case GGML_OP_SSM_SCAN:
            mi_op_ssm_scan(desc(node), desc(a), desc(b), desc(node->src[2]), desc(node->src[3]), desc(node->src[4]), desc(node->src[5]),
                           desc(node->src[6]), st);
            break;
        case GGML_OP_CPY:
        case GGML_OP_DUP:
        case GGML_OP_CONT:
            MI_ASSERT(ggml_nelements(node) == ggml_nelements(a));
            if (q8_quant_of(node->type) != MI_ACT_NONE) {
                mi_quantize_rows_q8(src_cols(a), a->ne[0], q8_quant_of(node->type), src_cols(node), st);
                break;
            }
            mi_op_cpy(desc(node), desc(a), st);
            break;
        case GGML_OP_ROPE: {
            const int32_t * pp = (const int32_t *) node->op_params;
            const int n_dims = pp[1], mode = pp[2], n_orig_ctx = pp[4];
            const float freq_base = op_param_f(node, 5), freq_scale = op_param_f(node, 6), ext_factor = op_param_f(node, 7);
            const float attn_factor = op_param_f(node, 8), beta_fast = op_param_f(node, 9), beta_slow = op_param_f(node, 10);
            MI_ASSERT(n_dims <= a->ne[0] && n_dims % 2 == 0);
            float corr[2];
            rope_corr_dims(n_dims, n_orig_ctx, freq_base, beta_fast, beta_slow, corr);
            const auto * tab = rope_table_find(ctx, n_dims, (int) a->ne[0], mode, freq_base, freq_scale, ext_factor, attn_factor, corr);
            mi_op_rope(desc(node), desc(a), (const int32_t *) b->data, n_dims, mode, freq_base, freq_scale, ext_factor,
                       attn_factor, corr[0], corr[1], tab ? tab->dev : nullptr, tab ? tab->P : 0, st);
            break;
        }
        default:
            fprintf(stderr, "%s: error: op not supported %s (%s)\\n", __func__, node->name, ggml_op_desc(node));
            MI_ASSERT(!"unsupported op");
    }
    ctx->last_launches++;
}

// GGML_OP_FLASH_ATTN_EXT (flash_attn.hip): reads src[0..3] where they lie -- no converted copy of any
// of them is made or cached -- and writes dst; the partials of a split KV range come from the graph's
// scratch (graph_scratch_bytes), a region of its own per node
mi_fa_desc fa_desc(const ggml_tensor * node) {
    const ggml_tensor * q = node->src[0];
    const ggml_tensor * k = node->src[1];
    const ggml_tensor * v = node->src[2];
    const ggml_tensor * mask = node->src[3];
    mi_fa_desc d = {};
    d.q = (const char *) q->data;
    d.k = (const char *) k->data;
    d.v = (const char *) v->data;
    d.mask = mask ? (const char *) mask->data : nullptr;
    d.dst = (float *) node->data;
    d.D = (int) q->ne[0];
    d.N = (int) q->ne[1];
    d.nh = (int) q->ne[2];
    d.ne3 = (int) q->ne[3];
    d.kv = (int) k->ne[1];
    d.nh_k = (int) k->ne[2];
    d.nh_v = (int) v->ne[2];
    d.ne3_k = (int) k->ne[3];
    d.ne3_v = (int) v->ne[3];
    d.nbq1 = q->nb[1]; d.nbq2 = q->nb[2]; d.nbq3 = q->nb[3];
    d.nbk1 = k->nb[1]; d.nbk2 = k->nb[2]; d.nbk3 = k->nb[3];
    d.nbv1 = v->nb[1]; d.nbv2 = v->nb[2]; d.nbv3 = v->nb[3];
    d.nbm1 = mask ? mask->nb[1] : 0;
    d.scale = op_param_f(node, 0);
    d.max_bias = op_param_f(node, 1);
    return d;
}

void op_flash_attn_ext(mi_backend_ctx * ctx, ggml_tensor * node) {
    const ggml_tensor * q = node->src[0];
    const ggml_tensor * k = node->src[1];
    const ggml_tensor * v = node->src[2];
    const ggml_tensor * mask = node->src[3];
    MI_ASSERT(q->type == GGML_TYPE_F32 && q->nb[0] == sizeof(float) && k->type == GGML_TYPE_F16 && v->type == GGML_TYPE_F16);
    MI_ASSERT(k->nb[0] == 2 && v->nb[0] == 2 && mi_fa_head_size_ok(k->ne[0]) && q->ne[0] == k->ne[0] && v->ne[0] == k->ne[0]);
    MI_ASSERT(v->ne[1] == k->ne[1] && q->ne[2] % k->ne[2] == 0 && q->ne[2] % v->ne[2] == 0 && q->ne[3] % k->ne[3] == 0 && q->ne[3] % v->ne[3] == 0);
    MI_ASSERT(!mask || (mask->type == GGML_TYPE_F16 && ggml_is_contiguous(mask) && mask->ne[0] >= k->ne[1] && mask->ne[1] >= q->ne[1]));
    MI_ASSERT(node->type == GGML_TYPE_F32 && ggml_is_contiguous(node));
    // op_params[2], the precision: GGML_PREC_DEFAULT and GGML_PREC_F32 run the same f32-accumulating kernels
    mi_fa_desc d = fa_desc(node);
    const size_t part = mi_fa_part_bytes(d);
    if (part) d.part = (float *) scratch_take(ctx, part);
    ctx->last_launches += mi_flash_attn_ext(d, ctx->stream);
}
