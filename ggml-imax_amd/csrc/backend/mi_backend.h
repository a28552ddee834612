// mi_backend.h -- internal to csrc/backend (not installed): what the backend's translation units
// share. The interfaces they implement are ggml_backend_buffer_type_i / ggml_backend_buffer_i /
// ggml_backend_i (src/ggml-backend-impl.h:18-117 of NAIST-Archlab/ggml-imax @ v2).
//
// The backend only uses the generic ggml API (ggml_nbytes, ggml_backend_buffer_init, ...), so the same
// objects load into either the repo's runtime (csrc/core) or the reference libggml. Functions that
// cross files are declared here (hidden visibility, as the whole library); all others are static.

#pragma once

#include "ggml_abi.h"
#include "ggml-mi355x.h"
#include "../kernels/mi355x_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#define MI_CHECK(call)                                                                                  \
    do {                                                                                                \
        const hipError_t err_ = (call);                                                                 \
        if (err_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ggml-mi355x: %s failed at %s:%d: %s\n", #call, __FILE__, __LINE__,       \
                    hipGetErrorString(err_));                                                           \
            abort();                                                                                    \
        }                                                                                               \
    } while (0)

// the kernels' names of the ggml types (mi355x_types.h) are the ABI's values
static_assert(MI_TYPE_F32 == GGML_TYPE_F32 && MI_TYPE_F16 == GGML_TYPE_F16 && MI_TYPE_Q4_0 == GGML_TYPE_Q4_0 && MI_TYPE_Q4_1 == GGML_TYPE_Q4_1 &&
              MI_TYPE_Q5_0 == GGML_TYPE_Q5_0 && MI_TYPE_Q5_1 == GGML_TYPE_Q5_1 && MI_TYPE_Q8_0 == GGML_TYPE_Q8_0 && MI_TYPE_Q8_1 == GGML_TYPE_Q8_1 &&
              MI_TYPE_Q4_K == GGML_TYPE_Q4_K && MI_TYPE_Q5_K == GGML_TYPE_Q5_K && MI_TYPE_Q6_K == GGML_TYPE_Q6_K && MI_TYPE_Q8_K == GGML_TYPE_Q8_K &&
              MI_TYPE_Q2_K == GGML_TYPE_Q2_K && MI_TYPE_Q3_K == GGML_TYPE_Q3_K && MI_TYPE_IQ4_NL == GGML_TYPE_IQ4_NL &&
              MI_TYPE_IQ4_XS == GGML_TYPE_IQ4_XS && MI_TYPE_I32 == GGML_TYPE_I32 && MI_TYPE_BF16 == GGML_TYPE_BF16, "mi355x_types.h names ggml_type values");

static constexpr size_t kBufferAlign = 256;   // tensor alignment inside device buffers
static constexpr size_t kBufferSlack = 256;   // tail slack: kernels may over-read < 16 B past a row

static inline size_t align_up(size_t bytes) { return (bytes + kBufferAlign - 1) & ~(kBufferAlign - 1); }

// ---- the environment (ggml-mi355x.cpp): every GGML_MI355X_* variable the backend files read ------
// Read once, at the first use (as a rule when the process creates its first backend). Two variables
// are read at a time of their own and so are no fields: GGML_MI355X_AUTOREGISTER (when the library is loaded) and
// GGML_MI355X_SPLIT_SLOTS (mi_env_split_slots).
struct mi_env_t {
    bool perf;             // GGML_MI355X_PERF: backends start with the per-node timer on
    bool no_mmq;           // GGML_MI355X_NO_MMQ: no prompt GEMM, prompts run on the GEMVs
    bool no_fused_mmv;     // GGML_MI355X_NO_FUSED_MMV: no quantize-in-kernel GEMV -- grouped launches, the
                           // MUL_MAT_ID stream path and fusion 32 below
    bool no_node_fusion;   // GGML_MI355X_NO_NODE_FUSION: every node its own launch
    // GGML_MI355X_FUSE_MASK (default 0x1ff), the enabled node fusions (debug / A-B): 1 norm, 2 softmax,
    // 4 f16 GEMV, 8 copies, 16 attention, 32 quantized GEMV epilogue / norm prologue, 64 embedding,
    // 128 attention + output projection, 256 mixture-of-experts router chain (also set_tuning fuse_router)
    int fuse_mask;
    bool debug_fusion;     // GGML_MI355X_DEBUG_FUSION: the attention planner says why it skips a block
    bool no_prefill_group; // GGML_MI355X_NO_PREFILL_GROUP: prompt GEMMs one by one
    bool disable_graphs;   // GGML_MI355X_DISABLE_GRAPHS: never capture
    int graph_min_launches;  // GGML_MI355X_GRAPH_MIN_LAUNCHES (4): smaller graphs are not worth a replay
    int plan_flush;        // GGML_MI355X_PLAN_FLUSH (A/B, 0): see mi_graph_plan_compute
    bool register_host;    // GGML_MI355X_REGISTER_HOST: register_host_buffer pins the caller's memory
};
const mi_env_t & mi_env();
int mi_env_split_slots();  // GGML_MI355X_SPLIT_SLOTS, read at the first split buffer type (0: unset)

// ---- devices, buffers (buffers.cpp) ---------------------------------------------------------------

int device_count();

struct mi_device_guard {
    int prev = -1;
    explicit mi_device_guard(int dev) {
        MI_CHECK(hipGetDevice(&prev));
        if (prev != dev) MI_CHECK(hipSetDevice(dev));
    }
    ~mi_device_guard() {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void) hipSetDevice(prev);
    }
};

struct mi_buffer_ctx {
    int device;
    void * dev_ptr;
    std::string name;
};
struct mi_split_slice {
    int slot;
    int device;
    int64_t row_low, row_high;
    char * ptr;
};
struct mi_split_extra {
    std::vector<mi_split_slice> slices;
};

bool buffer_is_mi355x(ggml_backend_buffer_t buffer);
bool is_split_tensor(const ggml_tensor * t);
int split_slots();
int slot_device(int slot);

// ---- backend context --------------------------------------------------------------------------------

// The form a mul_mat's activation columns are converted to: how they are quantized (the weight
// type's vec_dot_type; MI_ACT_NONE: src1 is read as it lies, F32 weights) and how they are laid out.
// Valid pairs: q8_0 / q8_1 / q8_K in SOA; q8_0 / q8_K in MFMA; f16 in ROWS and BLOCKED; bf16 in ROWS.
// ROWS and BLOCKED hold f16 or bf16 elements only, never quantized activations.
enum mi_act_layout : int {
    MI_LAYOUT_SOA,      // the GEMVs' structure-of-arrays (mi_act_q8)
    MI_LAYOUT_ROWS,     // f16 / bf16 elements, row-major [ncols][K]
    MI_LAYOUT_BLOCKED,  // f16 elements, the F16 prompt GEMMs' K-blocked layout [K/16][ncols][16] (mmq.hip)
    MI_LAYOUT_MFMA,     // the int8-MFMA layouts of the exact prefill GEMMs (mi_act_mmx, mmq_exact.hip)
};
struct mi_act_format {
    mi_act_quant quant = MI_ACT_NONE;
    mi_act_layout layout = MI_LAYOUT_SOA;
    bool operator==(const mi_act_format & o) const { return quant == o.quant && layout == o.layout; }
    bool operator!=(const mi_act_format & o) const { return !(*this == o); }
};

struct mi_act_cache_entry {
    const void * data;   // src1 data
    size_t nbytes;
    mi_act_format format;
    int64_t ne[4];
    size_t nb[4];
    void * dev;          // converted activations in scratch
};

struct mi_backend_ctx {
    int device;
    std::string name;
    hipStream_t stream = nullptr;
    void * scratch = nullptr;
    size_t scratch_size = 0;
    size_t scratch_used = 0;
    std::vector<mi_act_cache_entry> act_cache;
    int last_launches = 0;
    uint16_t * tables = nullptr;  // device: exp, gelu, silu fp16 tables (3 x 65536)
    hipEvent_t split_ready = nullptr;  // src1 of a split mul_mat is ready on `stream`
    hipEvent_t plan_marker = nullptr;  // recorded behind each plan launch (mi_graph_plan_compute)
    uint64_t scratch_gen = 0;     // bumped whenever `scratch` is reallocated (captures refer to it)
    // hipGraph plans (mi_graph_plan_create): captured launches of a whole ggml graph
    bool graphs = true;
    std::vector<hipGraphExec_t> exec_pool;  // executable graphs of freed plans, for in-place update
    int graph_fail_streak = 0;         // consecutive re-instantiations (update refused)
    // counters: [0] captures (plans and graph_compute), [1] instantiations, [2] in-place updates,
    // [3] direct (uncaptured) computes, [4] graph_compute replays of a cached capture,
    // [5] graph_compute captures
    int64_t graph_stats[6] = {};
    // graph_compute's own captures (ggml-cuda.cu:2456-2713 analogue): executable graphs keyed by
    // the exact launch-relevant content of the cgraph (mi_graph_key); an entry whose topology
    // matches a new graph is updated in place (hipGraphExecUpdate) before a new one is built
    struct gcache_entry {
        std::vector<uint64_t> key;
        uint64_t topo = 0;
        hipGraphExec_t exec = nullptr;
        hipEvent_t done = nullptr;  // recorded behind every launch of `exec`
        uint64_t last_use = 0;
        int launches = 0;
        bool no_update = false;  // hipGraphExecUpdate refused once: replay-only
    };
    // per-node timer (the reference's GGML_PERF, ggml.c:19195-19205): HIP events around every
    // dispatch unit of a directly launched graph; see ggml_backend_mi355x_set_perf
    bool perf = mi_env().perf;
    std::vector<hipEvent_t> perf_ev;   // pool
    std::vector<int> perf_at;          // node index at which unit k starts
    std::vector<gcache_entry> gcache;
    uint64_t gclock = 0;
    std::unordered_map<uint64_t, int> topo_launches;  // kernel launches of a topology's last direct run
    std::unordered_map<uint64_t, int> topo_misses;    // consecutive captures of a topology without a replay
    // host-built RoPE {cos, sin} tables (rope_table_ensure), one per parameter set
    struct rope_table {
        int n_dims, ne0, mode, P;
        float freq_base, freq_scale, ext_factor, attn_factor, corr0, corr1;
        float * dev;
    };
    std::vector<rope_table> rope_tables;
    // a node value still held as partial sums (try_fuse_attn_proj): `out` = sum_h parts[h], to be
    // stored by its consumer's kernel (the next GEMV's norm prologue) or by mi_sum_parts
    struct {
        const ggml_tensor * out = nullptr;
        float * parts = nullptr;
        int nparts = 0;
        int64_t n = 0;
    } pend;
};

// Scratch is sized once per graph (graph_scratch_bytes, graph.cpp) and only taken from after that.
void scratch_reserve(mi_backend_ctx * ctx, size_t bytes);
static inline void * scratch_take(mi_backend_ctx * ctx, size_t bytes) {
    bytes = align_up(bytes);
    MI_ASSERT(ctx->scratch_used + bytes <= ctx->scratch_size);
    void * p = (char *) ctx->scratch + ctx->scratch_used;
    ctx->scratch_used += bytes;
    return p;
}

// ---- small shared predicates ------------------------------------------------------------------------

// every row of the weight-type table has a mul_mat
static inline bool mm_src0_supported(ggml_type t) { return mi_type(t).type == t; }
static inline bool is_f32(const ggml_tensor * t) { return t && t->type == GGML_TYPE_F32; }
static inline bool is_f16_or_f32(const ggml_tensor * t) { return t && (t->type == GGML_TYPE_F32 || t->type == GGML_TYPE_F16); }

// the quantized vec_dot_type a src1 may already have for weight type t (GGML_TYPE_COUNT: none)
static inline ggml_type q8_src1_type(ggml_type t) {
    const mi_act_quant q = mi_type(t).act;
    return q == MI_ACT_NONE || q == MI_ACT_F16 || q == MI_ACT_BF16 ? GGML_TYPE_COUNT : (ggml_type) mi_act_type(q);
}

// the q8 quantization whose rows have type t (MI_ACT_NONE: t is no such type)
static inline mi_act_quant q8_quant_of(ggml_type t) {
    for (const mi_act_quant q : {MI_ACT_Q8_0, MI_ACT_Q8_1, MI_ACT_Q8_K})
        if (mi_act_type(q) == t) return q;
    return MI_ACT_NONE;
}

static inline float op_param_f(const ggml_tensor * t, int i) {
    float v;
    memcpy(&v, (const int32_t *) t->op_params + i, sizeof(float));
    return v;
}

static inline bool is_noop(const ggml_tensor * node) {
    return ggml_is_empty(node) || node->op == GGML_OP_NONE || node->op == GGML_OP_RESHAPE || node->op == GGML_OP_VIEW ||
           node->op == GGML_OP_PERMUTE || node->op == GGML_OP_TRANSPOSE;
}

static inline bool overlaps(const ggml_tensor * a, const ggml_tensor * b) {
    const char * a0 = (const char *) a->data;
    const char * b0 = (const char *) b->data;
    return a0 < b0 + ggml_nbytes(b) && b0 < a0 + ggml_nbytes(a);
}

// a 2-D weight and 2-D f32 columns, the elements of each side by side
static inline bool plain_2d_pair(const ggml_tensor * w, const ggml_tensor * x) {
    return w->ne[2] == 1 && w->ne[3] == 1 && x->ne[2] == 1 && x->ne[3] == 1 && w->nb[0] == ggml_type_size(w->type) && x->nb[0] == sizeof(float);
}
// a MUL_MAT node of such a pair whose f32 output elements lie side by side too
static inline bool plain_2d_operands(const ggml_tensor * n) { return plain_2d_pair(n->src[0], n->src[1]) && n->nb[0] == sizeof(float); }
// f32 columns a kernel loads 16 bytes at a time: the data and the column stride
static inline bool f32_cols_aligned(const ggml_tensor * x) { return ((uintptr_t) x->data | x->nb[1]) % 16 == 0; }

// this cgraph is a view of one scheduler split (ggml_graph_view, ggml-backend.c:1549: size 0, no hash
// table), not a whole graph: see mi_uses below and graph_decode_order (graph.cpp)
static inline bool sched_split_view(const ggml_cgraph * g) { return g->size == 0 && g->visited_hash_table.size == 0; }

// A graph handed over by ggml_backend_sched is a view of one split: a tensor may also be read by a
// later split that this backend never sees, so no use count taken over the view proves an
// intermediate private and every node output is stored (`partial`).
struct mi_uses {
    std::unordered_map<const ggml_tensor *, int> n;
    bool partial = false;
    int of(const ggml_tensor * t) const {
        if (partial) return 1 << 20;
        auto it = n.find(t);
        return it == n.end() ? 0 : it->second;
    }
};

// ---- mul_mat.cpp ------------------------------------------------------------------------------------

mi_act_format act_format_of(ggml_type t);
size_t act_bytes(mi_act_format f, int64_t K, int64_t ncols);
mi_src_cols src_cols(const ggml_tensor * t);
void invalidate_activations(mi_backend_ctx * ctx, const ggml_tensor * written);
size_t mmid_tables_bytes(int64_t n_as, int64_t pairs);
const char * planes_of(mi_backend_ctx * ctx, const ggml_tensor * a, const ggml_tensor * b);
const char * q40r_of(mi_backend_ctx * ctx, const ggml_tensor * a);
void q40r_apply(mi_backend_ctx * ctx, mi_mmv_group & g, const ggml_tensor * const * w);
void mmv_group_for(mi_mmv_group & g, const ggml_tensor * w, size_t x_stride, int ncols, size_t out_stride);
bool fused_mv_eligible(const ggml_tensor * n);
int run_mul_mat(mi_backend_ctx * ctx, ggml_cgraph * g, int i);
void op_mul_mat_id(mi_backend_ctx * ctx, ggml_tensor * dst);
void op_mul_mat_split(mi_backend_ctx * ctx, ggml_tensor * dst);

// ---- ops.cpp ----------------------------------------------------------------------------------------

bool mi_supports_op(ggml_backend_t backend, const ggml_tensor * op);
bool mi_offload_op(ggml_backend_t backend, const ggml_tensor * op);
const uint16_t * op_tables(mi_backend_ctx * ctx);
mi_tensor_desc desc(const ggml_tensor * t);
void rope_table_ensure(mi_backend_ctx * ctx, const ggml_tensor * node);
void op_companion(mi_backend_ctx * ctx, ggml_tensor * node);
mi_fa_desc fa_desc(const ggml_tensor * node);
void op_flash_attn_ext(mi_backend_ctx * ctx, ggml_tensor * node);

// ---- fusion.cpp -------------------------------------------------------------------------------------

struct mi_attn_plan {
    int kqv;  // node index of KQV
    const ggml_tensor * merged;  // the absorbed cont node the kernel writes
    mi_attn_desc d;
    // Q is read through its source strides at the KQV node. The graph allocator considers that
    // source dead after the (absorbed) cont of Q, so `merged` may have been placed over it: then
    // Q is copied to the backend's scratch at the cont's position instead.
    int q_copy_at = -1;          // node index of the cont of Q, or -1
    mi_tensor_desc q_src;        // Q through its source strides, [D, N, H]
};

void count_uses(const ggml_cgraph * g, mi_uses & u);
// nodes already executed inside another node's fused kernel: the running graph's list (this thread's)
void set_absorbed(const std::vector<uint8_t> * nodes);
bool absorbed(int j);
int next_node(const ggml_cgraph * g, int i);  // the next node that launches: no no-op, not absorbed; -1 at the end
void flush_pending(mi_backend_ctx * ctx);
void plan_attention(const ggml_cgraph * g, const mi_uses & u, std::vector<uint8_t> & absorbed_nodes, std::vector<mi_attn_plan> & plans);
// both return the last node the launch covered, or -1 (nothing launched)
int try_fuse_attn_proj(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_attn_plan & pl, const mi_uses & u);
int try_fuse_node(mi_backend_ctx * ctx, ggml_cgraph * g, int i, const mi_uses & u, std::vector<uint8_t> & absorbed_nodes);

// ---- graph.cpp (the vtable's entries) ---------------------------------------------------------------

enum ggml_status mi_graph_compute(ggml_backend_t backend, ggml_cgraph * cgraph);
ggml_backend_graph_plan_t mi_graph_plan_create(ggml_backend_t backend, const ggml_cgraph * cgraph);
void mi_graph_plan_free(ggml_backend_t backend, ggml_backend_graph_plan_t plan);
enum ggml_status mi_graph_plan_compute(ggml_backend_t backend, ggml_backend_graph_plan_t plan);
