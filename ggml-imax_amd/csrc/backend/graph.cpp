// graph.cpp -- how the MI355X backend runs a ggml graph: the node pass that dispatches and fuses, its
// scratch, the per-node timer, and the hipGraph captures behind graph_compute and the graph plans
// (src/ggml-cuda.cu:2456-2713 analogue: capture at :2576, exec update at :2690).

#include "mi_backend.h"

// ---- scratch -------------------------------------------------------------------------------

static bool capturing(const mi_backend_ctx * ctx) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    MI_CHECK(hipStreamIsCapturing(ctx->stream, &cs));
    return cs != hipStreamCaptureStatusNone;
}

void scratch_reserve(mi_backend_ctx * ctx, size_t bytes) {
    if (bytes <= ctx->scratch_size) return;
    MI_ASSERT(!capturing(ctx) && "scratch must be reserved before a graph capture");
    MI_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->scratch) MI_CHECK(hipFree(ctx->scratch));
    const size_t want = std::max(bytes + bytes / 2, (size_t) 16 << 20);
    MI_CHECK(hipMalloc(&ctx->scratch, want));
    ctx->scratch_size = want;
    ctx->scratch_gen++;  // executable graphs captured against the old buffer must not run again
}

// All the scratch a pass over `cgraph` can take, whatever it decides at run time: the one place that
// sizes it. mi_graph_launch_nodes and prepare_for_capture reserve this much, and everything after
// only takes (scratch_take asserts the bound).
static size_t graph_scratch_bytes(const ggml_cgraph * cgraph) {
    size_t total = 0;
    for (int i = 0; i < cgraph->n_nodes; i++) {
        const ggml_tensor * n = cgraph->nodes[i];
        if (n->op == GGML_OP_MUL_MAT_ID) {
            // the converted activations and the grouping tables (whichever path runs)
            const ggml_tensor * b = n->src[1];
            const mi_act_format f = act_format_of(n->src[0]->type);
            if (f.quant != MI_ACT_NONE) total += align_up(act_bytes(f, b->ne[0], b->ne[1] * b->ne[2] * b->ne[3]));
            if (n->src[2]) total += mmid_tables_bytes(n->src[0]->ne[2], n->src[2]->ne[0] * n->src[2]->ne[1]);
            continue;
        }
        if (n->op == GGML_OP_FLASH_ATTN_EXT) {
            // the partials of a split KV range, per node: two nodes never share a live region
            total += align_up(mi_fa_part_bytes(fa_desc(n)));
            continue;
        }
        // the attention planner's Q copies (mi_attn_plan::q_copy_at): each replaces the cont of a Q and
        // has that node's size, so every CONT node's bytes bound them
        if (n->op == GGML_OP_CONT) total += align_up(ggml_nbytes(n));
        if (n->op != GGML_OP_MUL_MAT) continue;
        if (n->src[0]->type == GGML_TYPE_F16 && n->src[1]->ne[1] == 1) {
            // a possible attention output projection (whatever op merged the heads -- ggml_cont as
            // main-backend.cpp:603 or ggml_cpy as main-ctx.cpp:566): room for its per-head partial
            // sums (try_fuse_attn_proj; head dim >= 64, so at most K / 64 heads)
            total += align_up((size_t) (n->src[0]->ne[0] / 64) * n->src[0]->ne[1] * sizeof(float));
        }
        // The weight type's own format (q8 SoA, f16 / bf16 rows) always; plus, above 8 columns, the
        // layout of the type's prompt GEMM where it has one (mm_act_format: K-blocked f16 or the exact
        // GEMMs' MFMA layout) -- both counted, the choice is made at run time.
        const mi_act_format f = act_format_of(n->src[0]->type);
        if (f.quant == MI_ACT_NONE) continue;
        const ggml_tensor * b = n->src[1];
        const int64_t ncols = b->ne[1] * b->ne[2] * b->ne[3];
        total += align_up(act_bytes(f, b->ne[0], ncols));
        if (ncols > 8 && (f.quant == MI_ACT_F16 || mi_type(n->src[0]->type).mmqx)) {
            const mi_act_layout gemm = f.quant == MI_ACT_F16 ? MI_LAYOUT_BLOCKED : MI_LAYOUT_MFMA;
            total += align_up(act_bytes({f.quant, gemm}, b->ne[0], ncols));
        }
    }
    return total;
}

// builds the RoPE tables a graph needs (before any capture: the uploads are synchronous)
static void rope_tables_prepare(mi_backend_ctx * ctx, const ggml_cgraph * cgraph) {
    for (int i = 0; i < cgraph->n_nodes; i++) {
        const ggml_tensor * n = cgraph->nodes[i];
        if (n->op == GGML_OP_ROPE && n->src[0] && n->src[0]->type == GGML_TYPE_F32) rope_table_ensure(ctx, n);
        if (n->op == GGML_OP_MUL_MAT) (void) planes_of(ctx, n->src[0], n->src[1]);
        // (decode GEMVs of a tree-order graph: the Q4_0 weights' aligned copies)
        if (n->op == GGML_OP_MUL_MAT && n->src[1]->ne[1] == 1 && mi_mmv_order() == 0) (void) q40r_of(ctx, n->src[0]);
    }
}

// ---- graph execution -----------------------------------------------------------------------

// ---- per-node timer ----------------------------------------------------------------------------
// A dispatch unit is one pass of mi_graph_launch_nodes' loop: a node, or a fused chain of nodes
// run by one kernel. perf_mark records an event before each unit (after the store of partial sums
// an earlier unit deferred, which stays in that unit's time; nodes absorbed into another node's
// kernel get no mark); perf_finish records the end,
// waits for the stream and adds each unit's device time to the perf fields of its last node (the
// other nodes of a fused chain get a run with no time, as the reference's fused-away work would),
// and the whole graph's to the cgraph's (ggml.c:19907-19922). ggml_graph_print shows them.
static bool perf_active(const mi_backend_ctx * ctx) { return ctx->perf && !capturing(ctx); }

static void perf_mark(mi_backend_ctx * ctx, int i) {
    const size_t k = ctx->perf_at.size();
    if (k == ctx->perf_ev.size()) {
        hipEvent_t e;
        MI_CHECK(hipEventCreate(&e));
        ctx->perf_ev.push_back(e);
    }
    MI_CHECK(hipEventRecord(ctx->perf_ev[k], ctx->stream));
    ctx->perf_at.push_back(i);
}

static void perf_finish(mi_backend_ctx * ctx, ggml_cgraph * g, int64_t t_host0) {
    const size_t n = ctx->perf_at.size();
    perf_mark(ctx, g->n_nodes);
    MI_CHECK(hipEventSynchronize(ctx->perf_ev[n]));
    for (size_t k = 0; k < n; k++) {
        float ms = 0.0f;
        MI_CHECK(hipEventElapsedTime(&ms, ctx->perf_ev[k], ctx->perf_ev[k + 1]));
        const int lo = ctx->perf_at[k], hi = ctx->perf_at[k + 1];
        // the time goes to the unit's last node that is not executed inside another node's kernel
        // (absorbed nodes between two units ran in an earlier unit's kernel: a run, no time)
        int last = -1, last_any = -1;
        for (int j = lo; j < hi; j++) {
            if (is_noop(g->nodes[j])) continue;
            g->nodes[j]->perf_runs++;
            last_any = j;
            if (!absorbed(j)) last = j;
        }
        if (last < 0) last = last_any;
        if (last >= 0) {
            const int64_t us = (int64_t) llround(ms * 1000.0);
            g->nodes[last]->perf_time_us += us;
            g->nodes[last]->perf_cycles += us;  // (device time: no CPU cycles; microseconds here)
        }
    }
    float total = 0.0f;
    if (n) MI_CHECK(hipEventElapsedTime(&total, ctx->perf_ev[0], ctx->perf_ev[n]));
    g->perf_runs++;
    g->perf_time_us += (int64_t) llround(total * 1000.0);
    g->perf_cycles += ggml_time_us() - t_host0;  // host wall time of the call, microseconds
    ctx->perf_at.clear();
}

// mmv_order -1: the decode summation order of a graph. A quantized MUL_MAT whose src1 is computed
// in the graph re-quantizes it (quantize_row_q8_*: round(x / d)), so a 1-ulp difference upstream can
// move a quant by a whole step and the logits of a quantized model by ~1e-2
// (tests/test_gpt2.py::test_reference_quantized_gpt2_is_ulp_sensitive): such graphs run every decode
// reduction in the reference CPU's order (bit-identical), and so do graphs whose ARGSORT orders a
// computed value (below). Any other graph (F16 models, a mul_mat of input data) keeps the tree order,
// within 1e-5 of the reference per op.
// A split input of the reference scheduler is a NONE tensor holding a value another split computed
// (ggml_backend_sched_split_graph creates it with ggml_dup_tensor_layout, ggml-backend.c:1498-1523).
// It cannot be told from a true graph input by its own fields (flags are set only when n_copies > 1,
// names may be truncated), but the graph says where it came from: the scheduler hands a backend
// views of its splits (sched_split_view), and a full graph never holds such copies. So in a split
// view every NONE source counts as computed -- the reference order, bit-identical either way -- and
// in a full graph as input.
// BF16 weights count as F16 does (ggml_is_quantized is false for both): rounding an activation to bf16 turns a
// 1-ulp f32 difference into another value only where it crosses a rounding tie, about once in 2^16 values,
// against every value near a boundary for round(x / d) -- DESIGN section 22 has the measured deviation.
static int graph_decode_order(const ggml_cgraph * g) {
    const bool view = sched_split_view(g);
    for (int i = 0; i < g->n_nodes; i++) {
        const ggml_tensor * n = g->nodes[i];
        // An ARGSORT (a router's top-k) is the same kind of discrete decision: a 1-ulp difference in a
        // value it orders can exchange two experts, and every weight multiplied after it. So a graph
        // whose ARGSORT consumes a value the graph computes runs in the reference order as well.
        const bool requant = (n->op == GGML_OP_MUL_MAT || n->op == GGML_OP_MUL_MAT_ID) && ggml_is_quantized(n->src[0]->type);
        if (!requant && n->op != GGML_OP_ARGSORT) continue;
        const ggml_tensor * x = requant ? n->src[1] : n->src[0];
        while (x->view_src || x->op == GGML_OP_RESHAPE || x->op == GGML_OP_VIEW || x->op == GGML_OP_PERMUTE ||
               x->op == GGML_OP_TRANSPOSE) {
            x = x->view_src ? x->view_src : x->src[0];
        }
        if (x->op != GGML_OP_NONE || view) return 1;
    }
    return 0;
}

static enum ggml_status mi_graph_launch_nodes(mi_backend_ctx * ctx, ggml_cgraph * cgraph) {
    tl_mi_graph_order = graph_decode_order(cgraph);
    if (!capturing(ctx)) rope_tables_prepare(ctx, cgraph);
    scratch_reserve(ctx, graph_scratch_bytes(cgraph));  // (a no-op inside a capture: prepare_for_capture reserved the same)
    ctx->scratch_used = 0;
    ctx->act_cache.clear();
    ctx->last_launches = 0;
    const bool no_node_fusion = mi_env().no_node_fusion;
    const int fuse_mask = mi_env().fuse_mask;  // the enabled node fusions: the bits are listed at mi_env_t
    ctx->pend = {};
    mi_uses uses;
    std::vector<uint8_t> absorbed_nodes;
    std::vector<mi_attn_plan> attn;
    if (!no_node_fusion) {
        count_uses(cgraph, uses);
        if (fuse_mask & 16) plan_attention(cgraph, uses, absorbed_nodes, attn);
    }
    bool q_copies = false;
    for (auto & pl : attn) {
        if (pl.q_copy_at < 0) continue;
        q_copies = true;
        pl.d.q = (char *) scratch_take(ctx, (size_t) pl.d.D * pl.d.N * pl.d.H * sizeof(float));  // (counted as its CONT node)
        pl.d.q_nb[0] = sizeof(float);
        pl.d.q_nb[1] = (size_t) pl.d.D * sizeof(float);
        pl.d.q_nb[2] = (size_t) pl.d.D * pl.d.N * sizeof(float);
    }
    set_absorbed(&absorbed_nodes);
    size_t next_attn = 0;
    const bool perf = perf_active(ctx);
    const int64_t perf_t0 = perf ? ggml_time_us() : 0;
    ctx->perf_at.clear();
    for (int i = 0; i < cgraph->n_nodes; i++) {
        ggml_tensor * node = cgraph->nodes[i];
        if (q_copies && absorbed(i)) {
            for (const auto & pl : attn) {
                if (pl.q_copy_at != i) continue;
                if (perf) perf_mark(ctx, i);  // the Q copy: a unit of its own
                mi_tensor_desc dq = pl.q_src;
                dq.data = (char *) pl.d.q;
                for (int k = 0; k < 3; k++) dq.nb[k] = pl.d.q_nb[k];
                mi_op_cpy(dq, pl.q_src, ctx->stream);
                ctx->last_launches++;
            }
        }
        if (is_noop(node) || absorbed(i)) continue;
        if (ctx->pend.out) {
            // a value held as partial sums is stored before any node but its norm consumer runs
            const bool consumer = !no_node_fusion && (fuse_mask & 1) && (node->op == GGML_OP_NORM || node->op == GGML_OP_RMS_NORM) &&
                                  node->src[0] == ctx->pend.out;
            if (!consumer) flush_pending(ctx);  // (still timed with the unit that deferred it)
        }
        if (perf) perf_mark(ctx, i);
        if (next_attn < attn.size() && attn[next_attn].kqv == i) {
            const int lastp = (fuse_mask & 128) ? try_fuse_attn_proj(ctx, cgraph, i, attn[next_attn], uses) : -1;
            if (lastp < 0) {
                mi_attn_ordered(attn[next_attn].d, op_tables(ctx), ctx->stream);
                ctx->last_launches++;
            }
            invalidate_activations(ctx, attn[next_attn].merged);  // written here, at the KQV node
            for (int k = i + 1; k <= lastp; k++) invalidate_activations(ctx, cgraph->nodes[k]);
            if (lastp >= 0) i = lastp;
            next_attn++;
            continue;
        }
        if (node->op == GGML_OP_MUL_MAT && is_split_tensor(node->src[0])) {
            op_mul_mat_split(ctx, node);
            invalidate_activations(ctx, node);
            continue;
        }
        const int last = no_node_fusion ? -1 : try_fuse_node(ctx, cgraph, i, uses, absorbed_nodes);
        if (last >= 0) {
            for (int k = i; k <= last; k++) invalidate_activations(ctx, cgraph->nodes[k]);
            i = last;
            continue;
        }
        flush_pending(ctx);
        switch (node->op) {
            case GGML_OP_MUL_MAT:
                i = run_mul_mat(ctx, cgraph, i);  // (with the nodes after it that share its launch; outputs invalidated)
                continue;
            case GGML_OP_MUL_MAT_ID:
                // always its own launch(es): no fusion pass absorbs it or takes it as producer / consumer
                op_mul_mat_id(ctx, node);
                break;
            case GGML_OP_FLASH_ATTN_EXT:
                // its own launch(es) as well; reads src[0..3] in place, writes dst (invalidated below)
                op_flash_attn_ext(ctx, node);
                break;
            default:
                op_companion(ctx, node);
        }
        invalidate_activations(ctx, node);
    }
    flush_pending(ctx);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        set_absorbed(nullptr);
        fprintf(stderr, "%s: kernel launch failed: %s\n", __func__, hipGetErrorString(err));
        return GGML_STATUS_FAILED;
    }
    if (perf) perf_finish(ctx, cgraph, perf_t0);
    set_absorbed(nullptr);
    return GGML_STATUS_SUCCESS;
}

static bool graphs_enabled(const mi_backend_ctx * ctx) {
    return ctx->graphs && !mi_env().disable_graphs && !ctx->perf;  // the per-node timer needs direct launches
}

// a graph that can be captured: no split-buffer mul_mat (several streams, events, peer copies)
static bool graph_capturable(const ggml_cgraph * cgraph) {
    for (int i = 0; i < cgraph->n_nodes; i++) {
        const ggml_tensor * n = cgraph->nodes[i];
        if (n->op == GGML_OP_MUL_MAT && is_split_tensor(n->src[0])) return false;
    }
    return true;
}

// Everything the node pass does synchronously -- table uploads, scratch growth -- done up front,
// so that a capture of the pass only enqueues kernels on ctx->stream.
static void prepare_for_capture(mi_backend_ctx * ctx, const ggml_cgraph * cgraph) {
    tl_mi_graph_order = graph_decode_order(cgraph);  // (the graph's order decides which weight copies it needs)
    op_tables(ctx);
    rope_tables_prepare(ctx, cgraph);
    scratch_reserve(ctx, graph_scratch_bytes(cgraph));
}

// Captures the node pass of `cgraph` into a hipGraph (nullptr if something in it could not be
// captured; the backend then launches directly from now on). The stream may still be running
// earlier work: the capture records only what follows.
static hipGraph_t capture_pass(mi_backend_ctx * ctx, ggml_cgraph * cgraph) {
    MI_CHECK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const ggml_status st = mi_graph_launch_nodes(ctx, cgraph);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(ctx->stream, &graph);
    if (st != GGML_STATUS_SUCCESS || ec != hipSuccess || !graph) {
        (void) hipGetLastError();
        if (graph) (void) hipGraphDestroy(graph);
        ctx->graphs = false;
        return nullptr;
    }
    ctx->graph_stats[0]++;
    return graph;
}

// The exact launch-relevant content of a graph: per node its output address, op, type, flags,
// shape, strides, op_params, view source and every source's address, type, flags, shape and
// strides; plus the scratch buffer the captured kernels use and the tuning knobs that choose
// kernels. Two graphs with equal keys launch identical kernels with identical arguments.
static void graph_key(const mi_backend_ctx * ctx, const ggml_cgraph * g, std::vector<uint64_t> & k) {
    k.clear();
    k.reserve((size_t) g->n_nodes * 40 + 16);
    k.push_back((uint64_t) g->n_nodes);
    k.push_back((uint64_t) sched_split_view(g));  // mi_uses::partial
    k.push_back((uint64_t) (uintptr_t) ctx->scratch);
    k.push_back(ctx->scratch_gen);
    // captured long-prompt GEMMs bake in the repacked planes' addresses (mi_mmx_member::planes): a
    // planes entry created or dropped since (a weight buffer freed and another allocated at the same
    // address) must not replay a graph that reads freed planes
    k.push_back(mi_planes_generation());
    {
        uint64_t tw[(sizeof(mi_tuning) + 7) / 8] = {};
        memcpy(tw, &g_mi_tuning, sizeof(mi_tuning));
        for (uint64_t w : tw) k.push_back(w);
    }
    auto tensor = [&](const ggml_tensor * t) {
        k.push_back((uint64_t) (uintptr_t) t->data);
        // flags too: whether a node's value is stored or fused away depends on GGML_TENSOR_FLAG_OUTPUT
        k.push_back((uint64_t) t->type | ((uint64_t) t->op << 16) | ((uint64_t) (uint32_t) t->flags << 32));
        for (int d = 0; d < 4; d++) k.push_back((uint64_t) t->ne[d]);
        for (int d = 0; d < 4; d++) k.push_back((uint64_t) t->nb[d]);
    };
    for (int i = 0; i < g->n_nodes; i++) {
        const ggml_tensor * t = g->nodes[i];
        tensor(t);
        k.push_back((uint64_t) (uintptr_t) t->view_src);
        uint64_t pw[GGML_MAX_OP_PARAMS / 8];
        memcpy(pw, t->op_params, sizeof(pw));
        for (uint64_t w : pw) k.push_back(w);
        int ns = 0;
        for (int j = 0; j < GGML_MAX_SRC; j++) if (t->src[j]) ns = j + 1;
        k.push_back((uint64_t) ns);
        for (int j = 0; j < ns; j++) {
            if (t->src[j]) tensor(t->src[j]);
            else k.push_back(0);
        }
    }
}

// topology of a graph (ops, types, source counts): graphs that differ only in addresses, shapes
// or parameters -- a decode step at the next position -- share it, so the executable graph of one
// can be updated in place for the other
static uint64_t graph_topology(const ggml_cgraph * g) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix((uint64_t) g->n_nodes);
    for (int i = 0; i < g->n_nodes; i++) {
        const ggml_tensor * t = g->nodes[i];
        int ns = 0;
        for (int j = 0; j < GGML_MAX_SRC; j++) if (t->src[j]) ns = j + 1;
        mix((uint64_t) t->op | ((uint64_t) t->type << 8) | ((uint64_t) ns << 16) | ((uint64_t) (t->view_src != nullptr) << 24));
    }
    return h;
}

static constexpr size_t kGraphCacheEntries = 8;
static constexpr int kGraphMissDirect = 3;
static constexpr int kGraphRetry = 32;

// Updates the executable graph `exec` in place to what `graph` captured. False when the runtime
// refuses (the kernels changed, not only their arguments), with the error state cleared: `exec` is
// as it was, and what becomes of it is the caller's policy.
static bool exec_update(hipGraphExec_t exec, hipGraph_t graph) {
    hipGraphNode_t err_node = nullptr;
    hipGraphExecUpdateResult res;
    if (hipGraphExecUpdate(exec, graph, &err_node, &res) == hipSuccess && res == hipGraphExecUpdateSuccess) return true;
    (void) hipGetLastError();
    return false;
}

static void gcache_launch(mi_backend_ctx * ctx, mi_backend_ctx::gcache_entry & e) {
    MI_CHECK(hipGraphLaunch(e.exec, ctx->stream));
    MI_CHECK(hipEventRecord(e.done, ctx->stream));
    e.last_use = ++ctx->gclock;
    ctx->last_launches = e.launches;
}

// graph_compute (ggml-cuda.cu:2456-2713 analogue: capture at :2576, exec update at :2690, the
// GGML_CUDA_DISABLE_GRAPHS switch at :2462). A graph whose exact content (graph_key) was captured
// before is replayed with one hipGraphLaunch. Otherwise: the first graph of a topology runs
// directly (its launch count decides whether capturing it pays); a later one is captured, an
// executable graph of the same topology is updated in place when only kernel arguments changed,
// else a new one is instantiated (at most kGraphCacheEntries per backend, least recently used
// evicted). Anything that cannot be captured runs directly.
enum ggml_status mi_graph_compute(ggml_backend_t backend, ggml_cgraph * cgraph) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    mi_device_guard g(ctx->device);
    if (!graphs_enabled(ctx) || !graph_capturable(cgraph)) {
        ctx->graph_stats[3]++;
        return mi_graph_launch_nodes(ctx, cgraph);
    }
    // A topology whose graphs kept arriving with new kernel arguments and never replayed (a decode
    // step through graph_compute: the KV length moves every call) launches directly: a capture costs
    // a synchronous recording of every launch plus an update per call for nothing, where a direct
    // launch overlaps host and device. Decided after kGraphMissDirect (3) such captures in a row; the
    // key and the preparation are then skipped too. Measured on main-batched.cpp's decode loop
    // (bench gpt2_batched): 4.9 k tokens/s capturing every step vs 6.2-6.5 k direct.
    // The decision decays: every kGraphRetry-th direct run of such a topology looks its key up
    // again, and a replay (a graph that does repeat) resets the count; set_graph_capture resets all.
    const uint64_t topo = graph_topology(cgraph);
    bool direct_only = false;
    {
        auto m = ctx->topo_misses.find(topo);
        if (m != ctx->topo_misses.end() && m->second >= kGraphMissDirect) {
            m->second++;
            if ((m->second - kGraphMissDirect) % kGraphRetry != 0) {
                ctx->graph_stats[3]++;
                return mi_graph_launch_nodes(ctx, cgraph);
            }
            direct_only = true;
        }
    }
    prepare_for_capture(ctx, cgraph);
    static thread_local std::vector<uint64_t> key;
    graph_key(ctx, cgraph, key);
    for (auto & e : ctx->gcache) {
        if (e.key == key) {
            ctx->graph_stats[4]++;
            ctx->topo_misses[e.topo] = 0;
            gcache_launch(ctx, e);
            return GGML_STATUS_SUCCESS;
        }
    }
    if (direct_only) {
        ctx->graph_stats[3]++;
        return mi_graph_launch_nodes(ctx, cgraph);
    }
    auto seen = ctx->topo_launches.find(topo);
    // captures below graph_min_launches kernel launches are not worth a replay (one small graph launches
    // faster directly than through hipGraphLaunch)
    if (seen == ctx->topo_launches.end() || seen->second < mi_env().graph_min_launches) {
        ctx->graph_stats[3]++;
        const ggml_status st = mi_graph_launch_nodes(ctx, cgraph);
        ctx->topo_launches[topo] = ctx->last_launches;
        return st;
    }
    ctx->topo_misses[topo]++;  // (reset by a replay of this topology)
    hipGraph_t graph = capture_pass(ctx, cgraph);
    if (!graph) {
        ctx->graph_stats[3]++;
        return mi_graph_launch_nodes(ctx, cgraph);
    }
    ctx->graph_stats[5]++;
    const int launches = ctx->last_launches;
    // An executable graph of this topology that is not in flight is updated in place (never one
    // still running). In a decode loop every step has a new key (the KV length moves) and the
    // previous step's executable is usually still running: rather than wait for it, a second one
    // per topology is instantiated, and the two then alternate. An entry whose update was refused
    // (a changed kernel choice) is no longer tried for updates; it still replays its own key.
    mi_backend_ctx::gcache_entry * slot = nullptr;
    auto try_update = [&](mi_backend_ctx::gcache_entry & e) {
        if (exec_update(e.exec, graph)) {
            ctx->graph_stats[2]++;
            slot = &e;
        } else {
            e.no_update = true;
        }
    };
    int same_topo = 0;
    mi_backend_ctx::gcache_entry * busy = nullptr;
    for (auto & e : ctx->gcache) {
        if (e.topo != topo || e.no_update) continue;
        same_topo++;
        const hipError_t q = hipEventQuery(e.done);
        if (q == hipErrorNotReady) {
            (void) hipGetLastError();
            if (!busy || e.last_use < busy->last_use) busy = &e;
            continue;
        }
        MI_CHECK(q);
        try_update(e);
        break;
    }
    if (!slot && busy && same_topo >= 2) {
        MI_CHECK(hipEventSynchronize(busy->done));
        try_update(*busy);
    }
    if (!slot) {
        if (ctx->gcache.size() >= kGraphCacheEntries) {
            auto lru = std::min_element(ctx->gcache.begin(), ctx->gcache.end(),
                                        [](const auto & a, const auto & b) { return a.last_use < b.last_use; });
            MI_CHECK(hipEventSynchronize(lru->done));
            MI_CHECK(hipGraphExecDestroy(lru->exec));
            MI_CHECK(hipEventDestroy(lru->done));
            ctx->gcache.erase(lru);
        }
        ctx->gcache.emplace_back();
        slot = &ctx->gcache.back();
        MI_CHECK(hipGraphInstantiate(&slot->exec, graph, nullptr, nullptr, 0));
        MI_CHECK(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
        ctx->graph_stats[1]++;
    }
    MI_CHECK(hipGraphDestroy(graph));
    slot->key = key;
    slot->topo = topo;
    slot->launches = launches;
    gcache_launch(ctx, *slot);
    return GGML_STATUS_SUCCESS;
}

// Graph plans (ggml_backend_graph_plan_create / _compute, ggml-backend.h): a plan is the graph's
// launches captured into a hipGraph, so computing it is one hipGraphLaunch instead of one host
// launch per kernel (~3 us each). A caller that knows its next graph early -- a decode loop,
// whose next graph depends on positions only -- creates the plan while the device still runs the
// current one. Executable graphs are pooled per backend: a new plan updates a pooled one in place
// (hipGraphExecUpdate) when only kernel arguments changed (KV length, cache offsets), and
// instantiates otherwise.
struct mi_graph_plan {
    ggml_cgraph graph;              // the caller's graph (node arrays stay the caller's)
    hipGraphExec_t exec = nullptr;  // null: launched directly at compute time
    uint64_t scratch_gen = 0;       // the scratch buffer generation the capture refers to
    int launches = 0;
};

// consecutive refused updates after which a backend stops capturing (as ggml-cuda.cu's
// disable_due_to_too_many_updates)
static constexpr int kGraphMaxFailStreak = 4;

ggml_backend_graph_plan_t mi_graph_plan_create(ggml_backend_t backend, const ggml_cgraph * cgraph) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    mi_device_guard g(ctx->device);
    auto * plan = new mi_graph_plan();
    plan->graph = *cgraph;
    if (!graphs_enabled(ctx) || !graph_capturable(cgraph)) return plan;
    prepare_for_capture(ctx, cgraph);
    hipGraph_t graph = capture_pass(ctx, &plan->graph);
    if (!graph) return plan;
    plan->scratch_gen = ctx->scratch_gen;
    plan->launches = ctx->last_launches;
    while (!ctx->exec_pool.empty() && !plan->exec) {
        hipGraphExec_t ex = ctx->exec_pool.back();
        ctx->exec_pool.pop_back();
        if (exec_update(ex, graph)) plan->exec = ex;
        else MI_CHECK(hipGraphExecDestroy(ex));
    }
    if (plan->exec) {
        ctx->graph_stats[2]++;
        ctx->graph_fail_streak = 0;
    } else {
        MI_CHECK(hipGraphInstantiate(&plan->exec, graph, nullptr, nullptr, 0));
        ctx->graph_stats[1]++;
        if (ctx->graph_stats[1] > 2 && ++ctx->graph_fail_streak >= kGraphMaxFailStreak) ctx->graphs = false;
    }
    MI_CHECK(hipGraphDestroy(graph));
    return plan;
}

void mi_graph_plan_free(ggml_backend_t backend, ggml_backend_graph_plan_t p) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    auto * plan = (mi_graph_plan *) p;
    if (plan->exec) {
        // kept for the next plan to update in place (at most a few per backend)
        if (ctx->exec_pool.size() < 4) ctx->exec_pool.push_back(plan->exec);
        else MI_CHECK(hipGraphExecDestroy(plan->exec));
    }
    delete plan;
}

enum ggml_status mi_graph_plan_compute(ggml_backend_t backend, ggml_backend_graph_plan_t p) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    auto * plan = (mi_graph_plan *) p;
    mi_device_guard g(ctx->device);
    // a plan captured against a scratch buffer that has since been reallocated (a later, larger
    // graph) would launch on freed memory: such a plan runs its nodes directly
    if (!plan->exec || plan->scratch_gen != ctx->scratch_gen) {
        ctx->graph_stats[3]++;
        return mi_graph_launch_nodes(ctx, &plan->graph);
    }
    MI_CHECK(hipGraphLaunch(plan->exec, ctx->stream));
    // GGML_MI355X_PLAN_FLUSH (A/B): 1 = a marker event behind the launch, 2 = hipStreamQuery, 0 (the
    // default) = nothing; no variant was faster than the noise in the GPT-2 decode loop (r03y2)
    const int flush = mi_env().plan_flush;
    if (flush == 1) {
        if (!ctx->plan_marker) MI_CHECK(hipEventCreateWithFlags(&ctx->plan_marker, hipEventDisableTiming));
        MI_CHECK(hipEventRecord(ctx->plan_marker, ctx->stream));
    } else if (flush == 2) {
        (void) hipStreamQuery(ctx->stream);
    }
    ctx->last_launches = plan->launches;
    return GGML_STATUS_SUCCESS;
}
