// fusion.cpp -- the MI355X backend's node fusion: the passes that run a chain of graph nodes as one
// kernel, and the attention planner. Each fused step is rounded exactly as its own node would be.
// (The reference's device backends launch node by node, src/ggml-cuda.cu:2456-2713; nothing there
// corresponds to this file.)

#include "mi_backend.h"

// ---- node fusion ----
//
// Patterns of the GPT-2 / LLaMA graphs (examples/gpt-2/main-backend.cpp:442-717):
//   NORM|RMS_NORM -> MUL(., g[E]) -> ADD(., b[E])             one k_norm launch
//   MUL_MAT(F16, few cols) -> ADD(., bias[N]) [-> ADD(., resid) | -> GELU]   one GEMV launch
//   SCALE -> DIAG_MASK_INF -> SOFT_MAX                          one k_soft_max launch
// An intermediate may be skipped only if the next node is its sole consumer and it is not a graph
// output; views of a tensor count as consumers of it.

// uses(X) = edges (consumer node, src == X) + views of X; a view V of X that is itself consumed
// counts once for X (as the view) and once per consumer for V
void count_uses(const ggml_cgraph * g, mi_uses & u) {
    u.n.clear();
    u.partial = sched_split_view(g);
    for (int i = 0; i < g->n_nodes; i++) {
        const ggml_tensor * t = g->nodes[i];
        for (int s = 0; s < GGML_MAX_SRC; s++) {
            if (t->src[s]) u.n[t->src[s]]++;
        }
        if (t->view_src) u.n[t->view_src]++;
    }
}

// nodes already executed inside another node's fused kernel (filled per graph by plan_attention and
// try_fuse_router; mi_graph_launch_nodes sets the list for the pass and clears it behind it)
static thread_local const std::vector<uint8_t> * tl_absorbed = nullptr;

void set_absorbed(const std::vector<uint8_t> * nodes) { tl_absorbed = nodes; }

bool absorbed(int j) { return tl_absorbed && j < (int) tl_absorbed->size() && (*tl_absorbed)[j]; }

int next_node(const ggml_cgraph * g, int i) {
    for (int j = i + 1; j < g->n_nodes; j++) {
        if (!is_noop(g->nodes[j]) && !absorbed(j)) return j;
    }
    return -1;
}

static bool private_intermediate(const ggml_tensor * t, const mi_uses & u) {
    return u.of(t) == 1 && !(t->flags & GGML_TENSOR_FLAG_OUTPUT);
}

// a fused kernel may write `out` over an input only when both are the same elements (each lane
// reads its element before writing it); any other overlap would race across workgroups
static bool safe_alias(const ggml_tensor * out, const ggml_tensor * in) {
    if (!in || !overlaps(out, in)) return true;
    return out->data == in->data && ggml_are_same_shape(out, in) && memcmp(out->nb, in->nb, sizeof(out->nb)) == 0;
}

static bool is_vec_f32(const ggml_tensor * t, int64_t n) {
    return t && t->type == GGML_TYPE_F32 && t->ne[0] == n && t->ne[1] == 1 && t->ne[2] == 1 && t->ne[3] == 1 &&
           t->nb[0] == sizeof(float);
}

// ADD(x, other) or ADD(other, x): returns `other`, or null
static const ggml_tensor * add_operand(const ggml_tensor * add, const ggml_tensor * x) {
    if (add->op != GGML_OP_ADD) return nullptr;
    if (add->src[0] == x) return add->src[1];
    if (add->src[1] == x) return add->src[0];
    return nullptr;
}

static int try_fuse_softmax(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u) {
    ggml_tensor * sc = g->nodes[i];
    const int j = next_node(g, i);
    if (j < 0 || !private_intermediate(sc, u)) return -1;
    ggml_tensor * dm = g->nodes[j];
    if (dm->op != GGML_OP_DIAG_MASK_INF || dm->src[0] != sc) return -1;
    const int k = next_node(g, j);
    if (k < 0 || !private_intermediate(dm, u)) return -1;
    ggml_tensor * sm = g->nodes[k];
    if (sm->op != GGML_OP_SOFT_MAX || sm->src[0] != dm || sm->src[1] != nullptr || op_param_f(sm, 1) != 0.0f) return -1;
    const ggml_tensor * a = sc->src[0];
    if (a->type != GGML_TYPE_F32 || !ggml_is_contiguous(a) || !ggml_are_same_shape(a, sm)) return -1;
    if (!safe_alias(sm, a)) return -1;
    const int n_past = ((const int32_t *) dm->op_params)[0];
    mi_op_soft_max(desc(sm), desc(a), desc(nullptr), op_param_f(sm, 0), op_tables(ctx), op_param_f(sc, 0), n_past, ctx->stream);
    ctx->last_launches++;
    return k;
}

// The graph's nodes right after mul_mat g->nodes[i] that a GEMV epilogue absorbs: ADD(bias[N]),
// then ADD(resid) or GELU, then up to two CPY nodes of row views of the result (GPT-2's K/V cache
// writes, main-backend.cpp:556-561). Fills `e` (mi_f16_epilogue or mi_mmv_group::epilogue: same
// fields), *out_p = the node holding the final value; returns the last absorbed node, or -1.
template <class E>
static int collect_epilogue(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, const ggml_tensor * w,
                            const ggml_tensor * x, E & e, ggml_tensor ** out_p, const ggml_tensor ** bias_p,
                            const ggml_tensor ** res_p) {
    ggml_tensor * mm = g->nodes[i];
    const int64_t N = w->ne[1];
    const ggml_tensor * bias_t = nullptr, * res_t = nullptr;
    ggml_tensor * out = mm;
    int last = i;
    int j = next_node(g, i);
    if (j >= 0 && private_intermediate(mm, u)) {
        ggml_tensor * add = g->nodes[j];
        const ggml_tensor * bias = add_operand(add, mm);
        if (bias && is_vec_f32(bias, N) && ggml_are_same_shape(add, mm) && add->nb[0] == sizeof(float)) {
            e.bias = (const float *) bias->data;
            bias_t = bias;
            out = add;
            last = j;
            const int k = next_node(g, j);
            if (k >= 0 && private_intermediate(add, u)) {
                ggml_tensor * n2 = g->nodes[k];
                const ggml_tensor * res = add_operand(n2, add);
                if (res && res != add && res->type == GGML_TYPE_F32 && ggml_are_same_shape(res, add) && res->nb[0] == sizeof(float) &&
                    n2->nb[0] == sizeof(float) && ggml_are_same_shape(n2, add)) {
                    e.resid = (const char *) res->data;
                    e.resid_nb1 = res->nb[1];
                    res_t = res;
                    out = n2;
                    last = k;
                } else if (n2->op == GGML_OP_UNARY && ggml_get_unary_op(n2) == GGML_UNARY_OP_GELU && n2->src[0] == add &&
                           n2->type == GGML_TYPE_F32 && n2->nb[0] == sizeof(float) && ggml_are_same_shape(n2, add)) {
                    e.gelu_table = op_tables(ctx) + 65536;
                    out = n2;
                    last = k;
                }
            }
        }
    }
    if (out->type != GGML_TYPE_F32 || out->nb[0] != sizeof(float)) return -1;
    // the graph's CPY nodes of row views of `out` that follow right away (GPT-2 writes the K and V
    // rows of c_attn's output into its caches, main-backend.cpp:556-561): stored by the epilogue
    int ncopy = 0;
    for (int j = next_node(g, last); j >= 0 && ncopy < 2; j = next_node(g, j)) {
        ggml_tensor * cp = g->nodes[j];
        if (cp->op != GGML_OP_CPY) break;
        const ggml_tensor * v = cp->src[0];
        // a row view of `out`, or `out` itself (e.g. the logits copied into a host staging tensor)
        if ((v->view_src != out && v != out) || v->type != GGML_TYPE_F32 || v->nb[0] != sizeof(float) || v->view_offs % sizeof(float)) break;
        if (v->ne[2] != 1 || v->ne[3] != 1 || v->ne[1] != out->ne[1] || (v->ne[1] > 1 && v->nb[1] != out->nb[1])) break;
        const int64_t r0 = v == out ? 0 : (int64_t) (v->view_offs / sizeof(float));
        if (r0 + v->ne[0] > N) break;
        if (cp->type != GGML_TYPE_F32 || !ggml_is_contiguous(cp) || ggml_nelements(cp) != ggml_nelements(v)) break;
        if (overlaps(cp, w) || overlaps(cp, x) || overlaps(cp, out) || (bias_t && overlaps(cp, bias_t)) || (res_t && overlaps(cp, res_t))) break;
        if (ncopy == 1 && overlaps(cp, g->nodes[last])) break;
        e.copy[ncopy].row0 = r0;
        e.copy[ncopy].row1 = r0 + v->ne[0];
        e.copy[ncopy].ptr = (char *) cp->data;
        e.copy[ncopy].col_stride = (size_t) v->ne[0] * sizeof(float);
        ncopy++;
        last = j;
    }
    *out_p = out;
    *bias_p = bias_t;
    *res_p = res_t;
    return last;
}

// stores a value left as partial sums (ctx->pend) before anything else reads it
void flush_pending(mi_backend_ctx * ctx) {
    if (!ctx->pend.out) return;
    mi_sum_parts((float *) ctx->pend.out->data, ctx->pend.parts, ctx->pend.nparts, ctx->pend.n, ctx->stream);
    ctx->last_launches++;
    ctx->pend = {};
}

// pro / pro_x: the src1 of this mul_mat is the output of a norm chain (norm -> mul g -> add b)
// that the kernel computes itself from pro_x (pro->parts: pro_x is the pending partial-sum value)
static int try_fuse_f16_gemv(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, const mi_norm_prologue * pro = nullptr,
                             const ggml_tensor * pro_x = nullptr) {
    ggml_tensor * mm = g->nodes[i];
    const ggml_tensor * w = mm->src[0];
    const ggml_tensor * x = pro_x ? pro_x : mm->src[1];
    if (is_split_tensor(w)) return -1;
    if (w->type != GGML_TYPE_F16 || x->type != GGML_TYPE_F32) return -1;
    // plain 2-D operands, with x the chain's input where a prologue computes src1; the output's element
    // stride is asked of the chain's last node (collect_epilogue). F16 rows of 16 bytes (the F16 type has
    // no mmv_align for fused_weight_aligned); no alignment is asked of the columns
    if (!plain_2d_pair(w, x) || x->ne[1] > 8) return -1;
    if (w->nb[1] % 16 != 0 || (uintptr_t) w->data % 16 != 0) return -1;
    if (!mi_mul_mat_f16_fused_supported(w->ne[0], x->ne[1])) return -1;
    const int64_t N = w->ne[1];
    mi_f16_epilogue e;
    const ggml_tensor * bias_t = nullptr, * res_t = nullptr;
    ggml_tensor * out = mm;
    const int last = collect_epilogue(ctx, g, i, u, w, x, e, &out, &bias_t, &res_t);
    if (last < 0) return -1;
    // every workgroup reads all of X and W; resid/bias are read per element. When the graph
    // allocator has placed `out` over X (X's last reader is this mul_mat), X is first converted
    // into the backend's scratch so no workgroup can see it overwritten.
    if (overlaps(out, w)) return -1;
    if (bias_t && overlaps(out, bias_t)) return -1;
    if (res_t && !safe_alias(out, res_t)) return -1;
    const uint16_t * xh = nullptr;
    if (pro && (overlaps(out, x) || (x->nb[1] % sizeof(float)) != 0)) return -1;
    if (pro && pro->parts) {
        // only the tree-order kernel sums partials
        if (mi_mmv_order() != 0 || !mi_mul_mat_f16_fast_supported(w->ne[0], x->ne[1], src_cols(x), nullptr, *pro)) return -1;
        // x (stored by the first workgroup) must not be read by the others through the epilogue
        if ((bias_t && overlaps(x, bias_t)) || (res_t && overlaps(x, res_t))) return -1;
        mi_mul_mat_f16_fast(w->data, w->nb[1], w->ne[0], N, src_cols(x), nullptr, x->ne[1], (float *) out->data, out->nb[1], e, *pro,
                            ctx->stream);
        ctx->last_launches++;
        return last;
    }
    if (overlaps(out, x)) {
        uint16_t * tmp = (uint16_t *) scratch_take(ctx, act_bytes({MI_ACT_F16, MI_LAYOUT_ROWS}, w->ne[0], x->ne[1]));
        mi_convert_f16(src_cols(x), w->ne[0], tmp, ctx->stream);
        ctx->last_launches++;
        xh = tmp;
    }
    const mi_norm_prologue none;
    mi_mul_mat_f16_fused(w->data, w->nb[1], w->ne[0], N, src_cols(x), xh, x->ne[1], (float *) out->data, out->nb[1], e,
                         pro ? *pro : none, ctx->stream);
    ctx->last_launches++;
    return last;
}

// Q4_0/Q8_0/Q4_K/Q5_K decode GEMV with the graph's bias / residual / GELU and K/V row copies in
// the streaming kernel's store (a one-member k_mmv_stream group); -1 if nothing follows that it
// can absorb (then the node goes through the grouped path).
// pro / pro_x: as for try_fuse_f16_gemv (the norm chain producing src1, computed in the kernel)
static int try_fuse_q_gemv(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, const mi_norm_prologue * pro = nullptr,
                           const ggml_tensor * pro_x = nullptr) {
    ggml_tensor * mm = g->nodes[i];
    if (!fused_mv_eligible(mm)) return -1;
    const ggml_tensor * w = mm->src[0];
    const ggml_tensor * x = pro_x ? pro_x : mm->src[1];
    if (pro && (w->ne[0] > kMiMmvProMaxK || x->nb[1] % sizeof(float) != 0 || x->ne[1] != mm->src[1]->ne[1])) return -1;
    mi_mmv_group grp;
    if (pro) {
        grp.pro.g = pro->g;
        grp.pro.b = pro->b;
        grp.pro.eps = pro->eps;
        grp.pro.mode = pro->mode;
    }
    const ggml_tensor * bias_t = nullptr, * res_t = nullptr;
    ggml_tensor * out = mm;
    const int last = collect_epilogue(ctx, g, i, u, w, x, grp.epi, &out, &bias_t, &res_t);
    if (last < 0 || (last == i && !pro)) return -1;
    // every workgroup quantizes all of X in its prologue and reads resid/bias per element: the
    // output may not overlap W, X or the bias, and may alias the residual only element for element
    if (overlaps(out, w) || overlaps(out, x) || (bias_t && overlaps(out, bias_t)) || !safe_alias(out, res_t)) return -1;
    if (out->nb[1] % sizeof(float) != 0) return -1;
    mmv_group_for(grp, w, x->nb[1], (int) x->ne[1], out->nb[1]);
    grp.n = 1;
    grp.m[0].W = w->data;
    grp.m[0].X = (const char *) x->data;
    grp.m[0].dst = (float *) out->data;
    q40r_apply(ctx, grp, &w);
    mi_mul_mat_q_fused(grp, ctx->stream);
    ctx->last_launches++;
    return last;
}

static int try_fuse_norm(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u) {
    ggml_tensor * norm = g->nodes[i];
    const int64_t E = norm->ne[0];
    const int j = next_node(g, i);
    if (j < 0 || !private_intermediate(norm, u)) return -1;
    ggml_tensor * mul = g->nodes[j];
    if (mul->op != GGML_OP_MUL || mul->src[0] != norm || !is_vec_f32(mul->src[1], E) || !ggml_are_same_shape(mul, norm)) return -1;
    ggml_tensor * out = mul;
    const float * bias = nullptr;
    int last = j;
    const int k = next_node(g, j);
    if (k >= 0 && private_intermediate(mul, u)) {
        ggml_tensor * add = g->nodes[k];
        if (add->op == GGML_OP_ADD && add->src[0] == mul && is_vec_f32(add->src[1], E) && ggml_are_same_shape(add, mul)) {
            out = add;
            bias = (const float *) add->src[1]->data;
            last = k;
        }
    }
    if (out->type != GGML_TYPE_F32 || out->nb[0] != sizeof(float)) return -1;
    // norm chain feeding an F16 GEMV as its only consumer: one kernel for all of it
    const int m = next_node(g, last);
    if (m >= 0 && private_intermediate(out, u) && g->nodes[m]->op == GGML_OP_MUL_MAT && g->nodes[m]->src[1] == out &&
        norm->src[0]->type == GGML_TYPE_F32 && norm->src[0]->nb[0] == sizeof(float) && ggml_are_same_shape(norm->src[0], out)) {
        mi_norm_prologue pro;
        pro.g = (const float *) mul->src[1]->data;
        pro.b = bias;
        pro.eps = op_param_f(norm, 0);
        pro.mode = norm->op == GGML_OP_RMS_NORM ? 2 : 1;
        if (ctx->pend.out && ctx->pend.out == norm->src[0] && ctx->pend.n == E) {
            // the norm's input is still partial sums (try_fuse_attn_proj): added in the prologue,
            // stored by the GEMV's first workgroup
            mi_norm_prologue pp = pro;
            pp.parts = ctx->pend.parts;
            pp.nparts = ctx->pend.nparts;
            pp.store = (float *) ctx->pend.out->data;
            const int r = try_fuse_f16_gemv(ctx, g, m, u, &pp, norm->src[0]);
            if (r >= 0) {
                ctx->pend = {};
                return r;
            }
        }
        flush_pending(ctx);
        int r = try_fuse_f16_gemv(ctx, g, m, u, &pro, norm->src[0]);
        if (r < 0 && (mi_env().fuse_mask & 32)) r = try_fuse_q_gemv(ctx, g, m, u, &pro, norm->src[0]);
        if (r >= 0) return r;
    }
    flush_pending(ctx);
    if (!safe_alias(out, norm->src[0]) || overlaps(out, mul->src[1]) || (bias && overlaps(out, g->nodes[last]->src[1]))) return -1;
    mi_op_norm(desc(out), desc(norm->src[0]), op_param_f(norm, 0), norm->op == GGML_OP_RMS_NORM,
               (const float *) mul->src[1]->data, bias, ctx->stream);
    ctx->last_launches++;
    return last;
}

// ---- attention subgraph (examples/gpt-2/main-backend.cpp:552-608) -----------------------------
//   KQ = mul_mat(K, permute(cont(Q))); scale; diag_mask_inf; soft_max;
//   KQV = mul_mat(cont(permute(V)), soft_max); cont(permute(KQV))
// becomes one k_attn_ordered launch at the KQV node; the conts of Q and V and the KQ chain are
// absorbed (they only feed this block), reading Q, K, V through their source strides.


// byte range [lo, hi) touched by a strided [ne0, ne1, ne2] view
static void strided_range(const char * base, const int64_t * ne, const size_t * nb, int n, const char ** lo, const char ** hi) {
    size_t span = 4;
    for (int k = 0; k < n; k++) span += (size_t) (ne[k] - 1) * nb[k];
    *lo = base;
    *hi = base + span;
}

static int node_index(const ggml_cgraph * g, const ggml_tensor * t, const std::unordered_map<const ggml_tensor *, int> & idx) {
    auto it = idx.find(t);
    return it == idx.end() ? -1 : it->second;
}

// virtual strides of a PERMUTE view P of a CONT node C, read through C's source
static bool permute_of_cont_strides(const ggml_tensor * P, size_t nb[3], const char ** base) {
    if (P->op != GGML_OP_PERMUTE || P->ne[3] != 1) return false;
    const ggml_tensor * C = P->src[0];
    if (!C || C->op != GGML_OP_CONT || C->type != GGML_TYPE_F32) return false;
    const ggml_tensor * S = C->src[0];
    if (!S || S->type != GGML_TYPE_F32 || S->nb[0] != sizeof(float)) return false;
    size_t vc[4];
    if (ggml_are_same_shape(S, C)) {
        for (int k = 0; k < 4; k++) vc[k] = S->nb[k];
    } else if (S->ne[2] == 1 && S->ne[3] == 1 && C->ne[3] == 1 && C->ne[0] * C->ne[1] == S->ne[0] && C->ne[2] == S->ne[1]) {
        vc[0] = sizeof(float);
        vc[1] = (size_t) C->ne[0] * sizeof(float);
        vc[2] = S->nb[1];
        vc[3] = 0;
    } else {
        return false;
    }
    const int32_t * ax = (const int32_t *) P->op_params;
    size_t vp[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++) {
        if (ax[k] < 0 || ax[k] > 3) return false;
        vp[ax[k]] = vc[k];
    }
    for (int k = 0; k < 3; k++) nb[k] = vp[k];
    *base = (const char *) S->data;
    return true;
}

void plan_attention(const ggml_cgraph * g, const mi_uses & u, std::vector<uint8_t> & absorbed_nodes,
                           std::vector<mi_attn_plan> & plans) {
    plans.clear();
    absorbed_nodes = std::vector<uint8_t>(g->n_nodes, 0);
    std::unordered_map<const ggml_tensor *, int> idx;
    for (int i = 0; i < g->n_nodes; i++) idx[g->nodes[i]] = i;
    const bool dbg = mi_env().debug_fusion;
#define MI_ATTN_SKIP(why) { if (dbg && kqv->src[1] && kqv->src[1]->op == GGML_OP_SOFT_MAX) fprintf(stderr, "attn plan: node %d: %s\n", j, why); continue; }
    for (int j = 0; j < g->n_nodes; j++) {
        const ggml_tensor * kqv = g->nodes[j];
        if (kqv->op != GGML_OP_MUL_MAT || kqv->type != GGML_TYPE_F32) continue;
        const ggml_tensor * vt = kqv->src[0];
        const ggml_tensor * sm = kqv->src[1];
        if (!vt || vt->op != GGML_OP_CONT || vt->type != GGML_TYPE_F32 || u.of(vt) != 1) MI_ATTN_SKIP("check 1")
        const ggml_tensor * vsrc = vt->src[0];
        if (!vsrc || vsrc->type != GGML_TYPE_F32 || !ggml_are_same_shape(vsrc, vt)) MI_ATTN_SKIP("check 2")
        if (sm->op != GGML_OP_SOFT_MAX || sm->src[1] || op_param_f(sm, 1) != 0.0f || u.of(sm) != 1) MI_ATTN_SKIP("check 3")
        // the causal mask: diag_mask_inf(scale(KQ)) (single-sequence graphs), or scale(KQ) + mask with an
        // F32 [n_kv, N] mask tensor broadcast over heads (batched decode across sequences)
        const ggml_tensor * dm = sm->src[0];
        const ggml_tensor * mask = nullptr;
        if (dm->op == GGML_OP_ADD && dm->type == GGML_TYPE_F32 && dm->src[1] && dm->src[1]->type == GGML_TYPE_F32) mask = dm->src[1];
        else if (dm->op != GGML_OP_DIAG_MASK_INF) MI_ATTN_SKIP("check 4")
        if (u.of(dm) != 1) MI_ATTN_SKIP("check 4")
        const ggml_tensor * sc = dm->src[0];
        if (sc->op != GGML_OP_SCALE || u.of(sc) != 1) MI_ATTN_SKIP("check 5")
        const ggml_tensor * kq = sc->src[0];
        if (kq->op != GGML_OP_MUL_MAT || kq->type != GGML_TYPE_F32 || u.of(kq) != 1) MI_ATTN_SKIP("check 6")
        const ggml_tensor * K = kq->src[0];
        const ggml_tensor * Qp = kq->src[1];
        if (K->type != GGML_TYPE_F32 || K->ne[3] != 1 || Qp->type != GGML_TYPE_F32 || u.of(Qp) != 1) MI_ATTN_SKIP("check 7")
        const ggml_tensor * qc = Qp->src[0];
        if (!qc || u.of(qc) != 2) continue;  // the permute view only (src + view_src)
        // KQV consumer: permute -> cont (merged, contiguous)
        int jp = -1, jm = -1;
        for (int k = j + 1; k < g->n_nodes && jm < 0; k++) {
            const ggml_tensor * n = g->nodes[k];
            if (jp < 0 && n->op == GGML_OP_PERMUTE && n->src[0] == kqv) jp = k;
            else if (jp >= 0 && n->op == GGML_OP_CONT && n->src[0] == g->nodes[jp]) jm = k;
        }
        if (jp < 0 || jm < 0 || u.of(kqv) != 2 || u.of(g->nodes[jp]) != 1) MI_ATTN_SKIP("check 8")
        const ggml_tensor * P2 = g->nodes[jp];
        const ggml_tensor * M = g->nodes[jm];
        if (M->type != GGML_TYPE_F32 || !ggml_is_contiguous(M) || P2->ne[3] != 1) MI_ATTN_SKIP("check 9")

        mi_attn_desc d;
        const char * qbase = nullptr;
        if (!permute_of_cont_strides(Qp, d.q_nb, &qbase)) MI_ATTN_SKIP("check 10")
        d.q = qbase;
        d.D = (int) K->ne[0];
        d.n_kv = (int) K->ne[1];
        d.H = (int) Qp->ne[2];
        d.N = (int) Qp->ne[1];
        if (Qp->ne[0] != K->ne[0] || K->ne[2] == 0 || d.H % K->ne[2] != 0) MI_ATTN_SKIP("check 11")
        d.r2 = d.H / (int) K->ne[2];
        if (vt->ne[0] != d.n_kv || vt->ne[1] != d.D || vt->ne[2] != K->ne[2]) MI_ATTN_SKIP("check 12")
        if (!mi_attn_supported(d.D, d.n_kv)) MI_ATTN_SKIP("check 13")
        d.k = (const char *) K->data;
        d.v = (const char *) vsrc->data;
        for (int k = 0; k < 3; k++) {
            d.k_nb[k] = K->nb[k];
            d.v_nb[k] = vsrc->nb[k];
        }
        // KQV (d, t, h) -> merged: linear index in P2's (permuted) order, M contiguous
        const int32_t * ax = (const int32_t *) P2->op_params;
        const size_t c[4] = {1, (size_t) P2->ne[0], (size_t) (P2->ne[0] * P2->ne[1]), (size_t) (P2->ne[0] * P2->ne[1] * P2->ne[2])};
        bool ok = true;
        for (int k = 0; k < 3; k++) {
            if (ax[k] < 0 || ax[k] > 3) ok = false;
            else d.o_nb[k] = c[ax[k]] * sizeof(float);
        }
        if (!ok) MI_ATTN_SKIP("check 14")
        d.out = (char *) M->data;
        if (mask) {
            if (mask->ne[0] != d.n_kv || mask->ne[1] != d.N || mask->ne[2] != 1 || mask->ne[3] != 1 ||
                mask->nb[0] != sizeof(float) || !mask->data || mask == sc) MI_ATTN_SKIP("check 4m")
            d.mask = (const char *) mask->data;
            d.mask_nb1 = mask->nb[1];
            d.n_past = INT32_MAX / 2;  // never: the mask carries the causal structure
        } else {
            d.n_past = ((const int32_t *) dm->op_params)[0];
        }
        d.pre_scale = op_param_f(sc, 0);
        d.sm_scale = op_param_f(sm, 0);
        const int absorbed_ids[] = {node_index(g, vt, idx), node_index(g, qc, idx), node_index(g, kq, idx), node_index(g, sc, idx),
                                    node_index(g, dm, idx), node_index(g, sm, idx), jm};
        bool all = true;
        for (int a : absorbed_ids) all &= a >= 0;
        if (!all) MI_ATTN_SKIP("check 15")
        // the block writes M alone: a tensor the graph's user asked to keep must be computed by its own node
        bool kept = (kqv->flags | P2->flags) & GGML_TENSOR_FLAG_OUTPUT;
        for (const ggml_tensor * t : {vt, qc, Qp, kq, sc, dm, sm}) kept |= (t->flags & GGML_TENSOR_FLAG_OUTPUT) != 0;
        if (kept) MI_ATTN_SKIP("check 15o")
        // the fused kernel writes M while other workgroups still read Q, K, V
        const char * mlo = (const char *) M->data;
        const char * mhi = mlo + ggml_nbytes(M);
        const char * lo, * hi;
        const int64_t kne[3] = {K->ne[0], K->ne[1], K->ne[2]};
        strided_range(d.k, kne, d.k_nb, 3, &lo, &hi);
        if (lo < mhi && mlo < hi) MI_ATTN_SKIP("check 16")
        const int64_t vne[3] = {vsrc->ne[0], vsrc->ne[1], vsrc->ne[2]};
        strided_range(d.v, vne, d.v_nb, 3, &lo, &hi);
        if (lo < mhi && mlo < hi) MI_ATTN_SKIP("check 17")
        mi_attn_plan pl;
        pl.kqv = j;
        pl.merged = M;
        pl.d = d;
        const int64_t qne[3] = {d.D, d.N, d.H};
        strided_range(d.q, qne, d.q_nb, 3, &lo, &hi);
        if (lo < mhi && mlo < hi) {
            pl.q_copy_at = node_index(g, qc, idx);
            pl.q_src.data = (char *) d.q;
            pl.q_src.type = GGML_TYPE_F32;
            for (int k = 0; k < 3; k++) {
                pl.q_src.ne[k] = qne[k];
                pl.q_src.nb[k] = d.q_nb[k];
            }
            pl.q_src.ne[3] = 1;
            pl.q_src.nb[3] = 0;
        }
        // Q, K and V are now read at the KQV node instead of at cont(Q) (or the copy that replaces
        // it), KQ and cont(V): no node that still runs in between may write over them
        std::vector<uint8_t> mine(g->n_nodes, 0);
        for (int a : absorbed_ids) mine[a] = 1;
        auto clobbered = [&](int from, const char * xlo, const char * xhi) {
            for (int k = from + 1; k < j; k++) {
                const ggml_tensor * n = g->nodes[k];
                if (mine[k] || absorbed_nodes[k] || is_noop(n) || !n->data) continue;
                const char * nlo = (const char *) n->data;
                if (nlo < xhi && xlo < nlo + ggml_nbytes(n)) return true;
            }
            return false;
        };
        strided_range(d.k, kne, d.k_nb, 3, &lo, &hi);
        if (clobbered(node_index(g, kq, idx), lo, hi)) MI_ATTN_SKIP("check 18")
        strided_range(d.v, vne, d.v_nb, 3, &lo, &hi);
        if (clobbered(node_index(g, vt, idx), lo, hi)) MI_ATTN_SKIP("check 19")
        if (pl.q_copy_at < 0) {
            strided_range(d.q, qne, d.q_nb, 3, &lo, &hi);
            if (clobbered(node_index(g, qc, idx), lo, hi)) MI_ATTN_SKIP("check 20")
        }
        if (mask) {  // read at KQV instead of at the ADD; also must not overlap the merged output
            const char * mlo2 = (const char *) mask->data;
            const char * mhi2 = mlo2 + ggml_nbytes(mask);
            if (clobbered(node_index(g, dm, idx), mlo2, mhi2) || (mlo2 < mhi && mlo < mhi2)) MI_ATTN_SKIP("check 21")
        }
        for (int a : absorbed_ids) absorbed_nodes[a] = 1;
        plans.push_back(pl);
    }
#undef MI_ATTN_SKIP
}

// At an attention block's KQV node: the block, the F16 output projection consuming its merged
// output (GPT-2's c_proj, main-backend.cpp:610-620) and that projection's bias and residual ADDs
// as one k_attn_proj launch, whose result stays as per-head partial sums (ctx->pend) until its
// consumer adds them (tree-order decode mode only). Returns the last node covered, or -1.
int try_fuse_attn_proj(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_attn_plan & pl, const mi_uses & u) {
    if (mi_mmv_order() != 0 || g_mi_tuning.attn_variant != 0 || pl.d.N != 1) return -1;
    const int j = next_node(g, i);
    if (j < 0) return -1;
    ggml_tensor * mm = g->nodes[j];
    const ggml_tensor * M = pl.merged;
    if (mm->op != GGML_OP_MUL_MAT || mm->src[1] != M || u.of(M) != 1 || (M->flags & GGML_TENSOR_FLAG_OUTPUT)) return -1;
    const ggml_tensor * w = mm->src[0];
    if (is_split_tensor(w) || w->type != GGML_TYPE_F16 || w->ne[2] != 1 || w->ne[3] != 1 || w->nb[0] != 2) return -1;
    if (M->ne[0] != w->ne[0] || M->ne[1] != 1 || M->ne[2] != 1 || M->ne[3] != 1) return -1;
    if (!mi_attn_proj_supported(pl.d, w->ne[0], w->ne[1], w->nb[1], w->data)) return -1;
    const int64_t N = w->ne[1];
    const int k1 = next_node(g, j);
    if (k1 < 0 || !private_intermediate(mm, u)) return -1;
    ggml_tensor * a1 = g->nodes[k1];
    const ggml_tensor * bias = add_operand(a1, mm);
    if (!bias || !is_vec_f32(bias, N) || !ggml_are_same_shape(a1, mm) || a1->nb[0] != sizeof(float)) return -1;
    const int k2 = next_node(g, k1);
    if (k2 < 0 || !private_intermediate(a1, u)) return -1;
    ggml_tensor * a2 = g->nodes[k2];
    const ggml_tensor * res = add_operand(a2, a1);
    if (!res || res == a1 || !is_vec_f32(res, N) || !is_vec_f32(a2, N)) return -1;
    if ((size_t) pl.d.H * N * sizeof(float) > (size_t) (w->ne[0] / 64) * N * sizeof(float)) return -1;  // graph_scratch_bytes
    float * parts = (float *) scratch_take(ctx, (size_t) pl.d.H * N * sizeof(float));
    mi_attn_proj_desc p;
    p.W = (const uint8_t *) w->data;
    p.nb01 = w->nb[1];
    p.N = N;
    p.bias = (const float *) bias->data;
    p.resid = (const float *) res->data;
    p.parts = parts;
    mi_attn_proj(pl.d, p, ctx->stream);
    ctx->last_launches++;
    ctx->pend.out = a2;
    ctx->pend.parts = parts;
    ctx->pend.nparts = pl.d.H;
    ctx->pend.n = N;
    return k2;
}

static bool is_copy(const ggml_tensor * t) {
    return (t->op == GGML_OP_CPY || t->op == GGML_OP_DUP || t->op == GGML_OP_CONT) && is_f16_or_f32(t->src[0]) && is_f16_or_f32(t) &&
           ggml_nelements(t) == ggml_nelements(t->src[0]);
}

// GET_ROWS(a, ia), GET_ROWS(b, ib), ADD of the two (GPT-2's token + position embedding,
// main-backend.cpp:475-478) as one launch; the two row sets must be private intermediates
static int try_fuse_embedding(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u) {
    ggml_tensor * g1 = g->nodes[i];
    const int j = next_node(g, i);
    if (j < 0) return -1;
    ggml_tensor * g2 = g->nodes[j];
    const int k = next_node(g, j);
    if (k < 0 || g2->op != GGML_OP_GET_ROWS) return -1;
    ggml_tensor * add = g->nodes[k];
    if (add->op != GGML_OP_ADD || !((add->src[0] == g1 && add->src[1] == g2) || (add->src[0] == g2 && add->src[1] == g1))) return -1;
    if (!private_intermediate(g1, u) || !private_intermediate(g2, u)) return -1;
    for (const ggml_tensor * t : {(const ggml_tensor *) g1, (const ggml_tensor *) g2}) {
        if (t->type != GGML_TYPE_F32 || t->ne[2] != 1 || t->ne[3] != 1 || t->src[1]->ne[1] != 1 || t->src[1]->ne[2] != 1) return -1;
        if (t->src[0]->ne[2] != 1 || t->src[0]->ne[3] != 1) return -1;
    }
    if (!ggml_are_same_shape(g1, g2) || !ggml_are_same_shape(add, g1) || add->type != GGML_TYPE_F32 || add->nb[0] != sizeof(float)) return -1;
    // the output is written while the row tables and indices are read
    for (const ggml_tensor * t : {g1->src[0], g1->src[1], g2->src[0], g2->src[1]}) {
        if (overlaps(add, t)) return -1;
    }
    mi_op_get_rows_add(desc(add), desc(g1->src[0]), desc(g1->src[1]), desc(g2->src[0]), desc(g2->src[1]), ctx->stream);
    ctx->last_launches++;
    return k;
}

// The router of a mixture-of-experts layer as one launch (router.hip k_router), entered at its SOFT_MAX:
//   probs = soft_max(logits)                    no mask, scale 1, max_bias 0, at most 64 experts
//   order = argsort(probs, DESC); sel = view(order, first k of each row)
//   w     = get_rows(reshape_3d(probs, 1, n_expert, T), sel)
//   [ w2 = reshape_2d(w, k, T); s = sum_rows(w2); wn = div(w2, s) ]
// The chain's nodes need not be adjacent (the expert mul_mats that read `sel` usually sit between the
// top-k and the weights), so the later ones are found through their sources within a window and
// marked absorbed. They are then written earlier than their place in the graph: none of them may
// overlap anything that a node in between reads or writes (an allocator may have given a later
// tensor the memory of an earlier one that is still live). Every tensor is written in full, as its
// own node writes it -- except the argsort rows past k when the top-k view is the argsort's only
// reader. MUL_MAT_ID is neither absorbed nor a producer here.
static constexpr int kRouterWindow = 64;

static int try_fuse_router(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, std::vector<uint8_t> & absorbed_nodes) {
    if (!g_mi_tuning.fuse_router) return -1;
    ggml_tensor * sm = g->nodes[i];
    const ggml_tensor * logits = sm->src[0];
    if (sm->src[1] || op_param_f(sm, 0) != 1.0f || op_param_f(sm, 1) != 0.0f) return -1;
    const int64_t n_expert = sm->ne[0], T = sm->ne[1];
    if (n_expert > kMiRouterMaxExperts || sm->ne[2] != 1 || sm->ne[3] != 1) return -1;
    if (!is_f32(sm) || !is_f32(logits) || !ggml_is_contiguous(sm) || !ggml_is_contiguous(logits) || !safe_alias(sm, logits)) return -1;
    const int end = std::min(g->n_nodes, i + kRouterWindow);
    int i_as = -1, i_v = -1, i_r3 = -1, i_gr = -1, i_r2 = -1, i_sr = -1, i_dv = -1;
    for (int j = i + 1; j < end; j++) {
        const ggml_tensor * n = g->nodes[j];
        if (absorbed(j)) continue;
        if (i_as < 0 && n->op == GGML_OP_ARGSORT && n->src[0] == sm) i_as = j;
        else if (i_v < 0 && i_as >= 0 && n->op == GGML_OP_VIEW && n->src[0] == g->nodes[i_as]) i_v = j;
        else if (i_r3 < 0 && n->op == GGML_OP_RESHAPE && n->src[0] == sm && n->ne[0] == 1 && n->ne[1] == n_expert) i_r3 = j;
        else if (i_gr < 0 && i_v >= 0 && i_r3 >= 0 && n->op == GGML_OP_GET_ROWS && n->src[0] == g->nodes[i_r3] && n->src[1] == g->nodes[i_v]) i_gr = j;
        else if (i_r2 < 0 && i_gr >= 0 && n->op == GGML_OP_RESHAPE && n->src[0] == g->nodes[i_gr]) i_r2 = j;
        else if (i_sr < 0 && i_r2 >= 0 && n->op == GGML_OP_SUM_ROWS && n->src[0] == g->nodes[i_r2]) i_sr = j;
        else if (i_dv < 0 && i_sr >= 0 && n->op == GGML_OP_DIV && n->src[0] == g->nodes[i_r2] && n->src[1] == g->nodes[i_sr]) i_dv = j;
    }
    if (i_gr < 0) return -1;
    ggml_tensor * as = g->nodes[i_as];
    const ggml_tensor * v = g->nodes[i_v];
    const ggml_tensor * r3 = g->nodes[i_r3];
    ggml_tensor * gr = g->nodes[i_gr];
    const int64_t k = v->ne[0];
    if (((const int32_t *) as->op_params)[0] != (int32_t) GGML_SORT_ORDER_DESC || as->type != GGML_TYPE_I32 || !ggml_is_contiguous(as)) return -1;
    if (v->view_src != as || v->view_offs != 0 || v->type != GGML_TYPE_I32 || k < 1 || k > n_expert || v->ne[1] != T || v->ne[2] != 1 ||
        v->ne[3] != 1 || v->nb[0] != sizeof(int32_t) || v->nb[1] != as->nb[1]) return -1;
    if (r3->ne[2] != T || r3->ne[3] != 1 || r3->view_src != sm || r3->view_offs != 0) return -1;
    if (!is_f32(gr) || !ggml_is_contiguous(gr) || gr->ne[0] != 1 || gr->ne[1] != k || gr->ne[2] != T || gr->ne[3] != 1) return -1;
    const bool tail = i_dv >= 0;
    ggml_tensor * sr = tail ? g->nodes[i_sr] : nullptr;
    ggml_tensor * dv = tail ? g->nodes[i_dv] : nullptr;
    if (tail) {
        const ggml_tensor * r2 = g->nodes[i_r2];
        if (r2->ne[0] != k || r2->ne[1] != T || r2->ne[2] != 1 || r2->ne[3] != 1 || r2->view_src != gr || r2->view_offs != 0) return -1;
        if (!is_f32(sr) || !is_f32(dv) || !ggml_is_contiguous(sr) || !ggml_is_contiguous(dv) || !ggml_are_same_shape(dv, r2)) return -1;
    }
    // the written tensors: disjoint from each other and from the logits (soft_max in place excepted)
    const ggml_tensor * outs[5] = {sm, as, gr, sr, dv};
    const int at[5] = {i, i_as, i_gr, tail ? i_sr : -1, tail ? i_dv : -1};
    const int n_out = tail ? 5 : 3;
    for (int a = 0; a < n_out; a++) {
        if (a > 0 && overlaps(outs[a], logits)) return -1;
        for (int b = a + 1; b < n_out; b++) {
            if (overlaps(outs[a], outs[b])) return -1;
        }
    }
    // written ahead of their place: nothing a node in between touches may lie under them
    auto in_chain = [&](const ggml_tensor * t) {
        const ggml_tensor * root = t->view_src ? t->view_src : t;
        for (int a = 0; a < n_out; a++) {
            if (root == outs[a]) return true;
        }
        return false;
    };
    for (int a = 1; a < n_out; a++) {
        for (int j = i + 1; j < at[a]; j++) {
            const ggml_tensor * n = g->nodes[j];
            if (is_noop(n) || in_chain(n)) continue;
            if (overlaps(outs[a], n)) return -1;
            for (int s = 0; s < GGML_MAX_SRC; s++) {
                if (n->src[s] && n->src[s]->data && !in_chain(n->src[s]) && overlaps(outs[a], n->src[s])) return -1;
            }
        }
    }
    mi_router_desc r;
    r.logits = (const float *) logits->data;
    r.probs = (float *) sm->data;
    r.sorted = (int32_t *) as->data;
    r.weights = (float *) gr->data;
    r.sums = tail ? (float *) sr->data : nullptr;
    r.normed = tail ? (float *) dv->data : nullptr;
    r.n_expert = (int) n_expert;
    r.k = (int) k;
    // the rows' tails stay unwritten only where the top-k view is provably the argsort's one reader
    // (its two uses: the view's source and its view_src)
    r.n_sorted = u.of(as) == 2 && !(as->flags & GGML_TENSOR_FLAG_OUTPUT) ? (int) k : (int) n_expert;
    r.T = T;
    mi_router_fused(r, op_tables(ctx), ctx->stream);
    ctx->last_launches++;
    if (absorbed_nodes.size() < (size_t) g->n_nodes) absorbed_nodes.resize((size_t) g->n_nodes, 0);
    for (int a = 1; a < n_out; a++) {
        absorbed_nodes[at[a]] = 1;
        invalidate_activations(ctx, outs[a]);
    }
    return i;
}

// consecutive independent copies (GPT-2: K -> cache, V -> cache, cont(Q)) as one launch
static int try_fuse_copies(mi_backend_ctx * ctx, ggml_cgraph * g, int i) {
    std::vector<ggml_tensor *> grp = {g->nodes[i]};
    if (!is_copy(grp[0])) return -1;
    int last = i;
    for (int j = next_node(g, i); j >= 0 && (int) grp.size() < kMiMaxCopies; j = next_node(g, j)) {
        ggml_tensor * n = g->nodes[j];
        if (!is_copy(n)) break;
        bool indep = true;
        for (ggml_tensor * m : grp) {
            if (overlaps(n->src[0], m) || overlaps(n, m->src[0]) || overlaps(n, m)) indep = false;
        }
        if (!indep) break;
        grp.push_back(n);
        last = j;
    }
    if (grp.size() < 2) return -1;
    mi_tensor_desc d[kMiMaxCopies], a[kMiMaxCopies];
    for (size_t k = 0; k < grp.size(); k++) {
        d[k] = desc(grp[k]);
        a[k] = desc(grp[k]->src[0]);
    }
    mi_op_cpy_multi(d, a, (int) grp.size(), ctx->stream);
    ctx->last_launches++;
    return last;
}

// The fusion pass that starts at nodes[i], by its op and the enabled fusions (mi_env_t::fuse_mask):
// the last node its launch covered, or -1 (nothing launched).
int try_fuse_node(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, std::vector<uint8_t> & absorbed_nodes) {
    const int mask = mi_env().fuse_mask;
    int last = -1;
    switch (g->nodes[i]->op) {
        case GGML_OP_NORM:
        case GGML_OP_RMS_NORM: return (mask & 1) ? try_fuse_norm(ctx, g, i, u) : -1;
        case GGML_OP_SCALE: return (mask & 2) ? try_fuse_softmax(ctx, g, i, u) : -1;
        case GGML_OP_MUL_MAT:
            if (mask & 4) last = try_fuse_f16_gemv(ctx, g, i, u);
            if (last < 0 && (mask & 32)) last = try_fuse_q_gemv(ctx, g, i, u);
            return last;
        case GGML_OP_CPY:
        case GGML_OP_DUP:
        case GGML_OP_CONT: return (mask & 8) ? try_fuse_copies(ctx, g, i) : -1;
        case GGML_OP_GET_ROWS: return (mask & 64) ? try_fuse_embedding(ctx, g, i, u) : -1;
        case GGML_OP_SOFT_MAX: return (mask & 256) ? try_fuse_router(ctx, g, i, u, absorbed_nodes) : -1;
        default: return -1;
    }
}
