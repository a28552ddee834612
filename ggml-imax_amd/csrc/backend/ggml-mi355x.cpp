// ggml-mi355x.cpp -- the MI355X (gfx950) ggml backend: the environment, the backend vtable with its
// events, initialisation, registration and the public API of ggml-mi355x.h. The rest of the backend
// is beside it: buffers.cpp, mul_mat.cpp, ops.cpp, fusion.cpp, graph.cpp, declared in mi_backend.h.
//
// Implements ggml_backend_i (src/ggml-backend-impl.h:18-117 of NAIST-Archlab/ggml-imax @ v2) the
// way the reference's device backends do (structural analogue: src/ggml-cuda.cu:2870-2942
// events/vtable, :3024-3042 registration) -- but written for one process per GPU, HIP streams,
// wave64 kernels and activation quantization on the device.

#include "mi_backend.h"

#include <dlfcn.h>

// ---- the environment: the only reads of it in the backend files ----------------------------

static bool env_set(const char * name) { return getenv(name) != nullptr; }
static int env_int(const char * name, int unset) {
    const char * e = getenv(name);
    return e ? atoi(e) : unset;
}

const mi_env_t & mi_env() {
    static const mi_env_t env = {
        /* perf               */ env_set("GGML_MI355X_PERF"),
        /* no_mmq             */ env_set("GGML_MI355X_NO_MMQ"),
        /* no_fused_mmv       */ env_set("GGML_MI355X_NO_FUSED_MMV"),
        /* no_node_fusion     */ env_set("GGML_MI355X_NO_NODE_FUSION"),
        /* fuse_mask          */ env_int("GGML_MI355X_FUSE_MASK", 0x1ff) & (env_set("GGML_MI355X_NO_FUSED_MMV") ? ~32 : ~0),
        /* debug_fusion       */ env_set("GGML_MI355X_DEBUG_FUSION"),
        /* no_prefill_group   */ env_set("GGML_MI355X_NO_PREFILL_GROUP"),
        /* disable_graphs     */ env_set("GGML_MI355X_DISABLE_GRAPHS"),
        /* graph_min_launches */ env_int("GGML_MI355X_GRAPH_MIN_LAUNCHES", 4),
        /* plan_flush         */ env_int("GGML_MI355X_PLAN_FLUSH", 0),
        /* register_host      */ env_set("GGML_MI355X_REGISTER_HOST"),
    };
    return env;
}

int mi_env_split_slots() {
    static const int v = env_int("GGML_MI355X_SPLIT_SLOTS", 0);
    return v;
}

static ggml_guid_t mi_guid() {
    static ggml_guid guid = {0x4d, 0x49, 0x33, 0x35, 0x35, 0x58, 0x2d, 0x67, 0x66, 0x78, 0x39, 0x35, 0x30, 0x2d, 0x76, 0x31};
    return &guid;
}

// ---------------------------------------------------------------------------------------------
// backend vtable
// ---------------------------------------------------------------------------------------------

static const char * mi_backend_name(ggml_backend_t backend) { return ((mi_backend_ctx *) backend->context)->name.c_str(); }

static void mi_backend_free(ggml_backend_t backend) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    {
        mi_device_guard g(ctx->device);
        MI_CHECK(hipStreamSynchronize(ctx->stream));
        for (hipGraphExec_t ex : ctx->exec_pool) MI_CHECK(hipGraphExecDestroy(ex));
        for (auto & e : ctx->gcache) {
            MI_CHECK(hipGraphExecDestroy(e.exec));
            MI_CHECK(hipEventDestroy(e.done));
        }
        if (ctx->scratch) MI_CHECK(hipFree(ctx->scratch));
        if (ctx->tables) MI_CHECK(hipFree(ctx->tables));
        for (auto & t : ctx->rope_tables) MI_CHECK(hipFree(t.dev));
        if (ctx->plan_marker) MI_CHECK(hipEventDestroy(ctx->plan_marker));
        if (ctx->split_ready) MI_CHECK(hipEventDestroy(ctx->split_ready));
        for (hipEvent_t e : ctx->perf_ev) MI_CHECK(hipEventDestroy(e));
        MI_CHECK(hipStreamDestroy(ctx->stream));
    }
    delete ctx;
    delete backend;
}

static ggml_backend_buffer_type_t mi_backend_default_buft(ggml_backend_t backend) {
    return ggml_backend_mi355x_buffer_type(((mi_backend_ctx *) backend->context)->device);
}

static void mi_backend_set_tensor_async(ggml_backend_t backend, ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    ggml_backend_buffer_t buf = tensor->view_src ? tensor->view_src->buffer : tensor->buffer;
    MI_ASSERT(buffer_is_mi355x(buf) && "unsupported buffer type");
    mi_device_guard g(ctx->device);
    MI_CHECK(hipMemcpyAsync((char *) tensor->data + offset, data, size, hipMemcpyHostToDevice, ctx->stream));
    mi_planes_refresh((char *) tensor->data + offset, size, ctx->stream);  // repacked planes over these bytes, after the copy
}

static void mi_backend_get_tensor_async(ggml_backend_t backend, const ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    ggml_backend_buffer_t buf = tensor->view_src ? tensor->view_src->buffer : tensor->buffer;
    MI_ASSERT(buffer_is_mi355x(buf) && "unsupported buffer type");
    mi_device_guard g(ctx->device);
    MI_CHECK(hipMemcpyAsync(data, (const char *) tensor->data + offset, size, hipMemcpyDeviceToHost, ctx->stream));
}

static bool mi_backend_cpy_tensor_async(ggml_backend_t backend_src, ggml_backend_t backend_dst, const ggml_tensor * src, ggml_tensor * dst) {
    if (!ggml_backend_is_mi355x(backend_src) || !ggml_backend_is_mi355x(backend_dst)) return false;
    ggml_backend_buffer_t sbuf = src->view_src ? src->view_src->buffer : src->buffer;
    ggml_backend_buffer_t dbuf = dst->view_src ? dst->view_src->buffer : dst->buffer;
    if (!buffer_is_mi355x(sbuf) || !buffer_is_mi355x(dbuf)) return false;
    auto * cs = (mi_backend_ctx *) backend_src->context;
    auto * cd = (mi_backend_ctx *) backend_dst->context;
    if (cs->device == cd->device) {
        mi_device_guard g(cs->device);
        MI_CHECK(hipMemcpyAsync(dst->data, src->data, ggml_nbytes(dst), hipMemcpyDeviceToDevice, cd->stream));
        mi_planes_refresh(dst->data, ggml_nbytes(dst), cd->stream);
        return true;
    }
    // cross-device: copy on the source stream after its producers, destination waits on an event
    mi_device_guard g(cs->device);
    MI_CHECK(hipMemcpyPeerAsync(dst->data, cd->device, src->data, cs->device, ggml_nbytes(dst), cs->stream));
    hipEvent_t ev;
    MI_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    MI_CHECK(hipEventRecord(ev, cs->stream));
    {
        mi_device_guard g2(cd->device);
        MI_CHECK(hipStreamWaitEvent(cd->stream, ev, 0));
        mi_planes_refresh(dst->data, ggml_nbytes(dst), cd->stream);  // on the destination, behind the copy
    }
    MI_CHECK(hipEventDestroy(ev));
    return true;
}

static void mi_backend_synchronize(ggml_backend_t backend) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    mi_device_guard g(ctx->device);
    MI_CHECK(hipStreamSynchronize(ctx->stream));
}

static ggml_backend_event_t mi_event_new(ggml_backend_t backend) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    mi_device_guard g(ctx->device);
    hipEvent_t ev;
    MI_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    auto * e = new ggml_backend_event;
    e->backend = backend;
    e->context = ev;
    return e;
}

static void mi_event_free(ggml_backend_event_t event) {
    MI_CHECK(hipEventDestroy((hipEvent_t) event->context));
    delete event;
}

static void mi_event_record(ggml_backend_event_t event) {
    auto * ctx = (mi_backend_ctx *) event->backend->context;
    MI_CHECK(hipEventRecord((hipEvent_t) event->context, ctx->stream));
}

static void mi_event_wait(ggml_backend_t backend, ggml_backend_event_t event) {
    auto * ctx = (mi_backend_ctx *) backend->context;
    if (ggml_backend_is_mi355x(event->backend)) {
        MI_CHECK(hipStreamWaitEvent(ctx->stream, (hipEvent_t) event->context, 0));
    } else {
        event->backend->iface.event_synchronize(event);
    }
}

static void mi_event_synchronize(ggml_backend_event_t event) { MI_CHECK(hipEventSynchronize((hipEvent_t) event->context)); }

static const ggml_backend_i k_mi_backend_i = {
    /* get_name                */ mi_backend_name,
    /* free                    */ mi_backend_free,
    /* get_default_buffer_type */ mi_backend_default_buft,
    /* set_tensor_async        */ mi_backend_set_tensor_async,
    /* get_tensor_async        */ mi_backend_get_tensor_async,
    /* cpy_tensor_async        */ mi_backend_cpy_tensor_async,
    /* synchronize             */ mi_backend_synchronize,
    /* graph_plan_create       */ mi_graph_plan_create,
    /* graph_plan_free         */ mi_graph_plan_free,
    /* graph_plan_compute      */ mi_graph_plan_compute,
    /* graph_compute           */ mi_graph_compute,
    /* supports_op             */ mi_supports_op,
    /* offload_op              */ mi_offload_op,
    /* event_new               */ mi_event_new,
    /* event_free              */ mi_event_free,
    /* event_record            */ mi_event_record,
    /* event_wait              */ mi_event_wait,
    /* event_synchronize       */ mi_event_synchronize,
};

// ---------------------------------------------------------------------------------------------
// public API
// ---------------------------------------------------------------------------------------------

extern "C" {

int ggml_backend_mi355x_get_device_count(void) { return device_count(); }

void ggml_backend_mi355x_get_device_description(int device, char * description, size_t description_size) {
    hipDeviceProp_t prop;
    MI_CHECK(hipGetDeviceProperties(&prop, device));
    snprintf(description, description_size, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
}

void ggml_backend_mi355x_get_device_memory(int device, size_t * free, size_t * total) {
    mi_device_guard g(device);
    MI_CHECK(hipMemGetInfo(free, total));
}

bool ggml_backend_mi355x_register_host_buffer(void * buffer, size_t size) {
    if (!mi_env().register_host) return false;
    const hipError_t err = hipHostRegister(buffer, size, hipHostRegisterPortable | hipHostRegisterReadOnly);
    if (err != hipSuccess) {
        (void) hipGetLastError();
        return false;
    }
    return true;
}

void ggml_backend_mi355x_unregister_host_buffer(void * buffer) {
    if (!mi_env().register_host) return;
    (void) hipHostUnregister(buffer);
    (void) hipGetLastError();
}

} // extern "C"

// The reference's type traits (ggml.h ggml_type_traits_t), looked up in the library that this one's
// ggml_* references are bound to; the repo's own runtime exports none (null then).
struct mi_ggml_type_traits {
    const char * type_name;
    int blck_size;
    size_t type_size;
    bool is_quantized;
    void * to_float, * from_float, * from_float_reference, * vec_dot;
    enum ggml_type vec_dot_type;
    int64_t nrows;
};
typedef mi_ggml_type_traits (*mi_get_type_traits_t)(enum ggml_type);
static mi_get_type_traits_t bound_type_traits() {
    Dl_info info;
    if (!dladdr((void *) &ggml_type_size, &info) || !info.dli_fname) return nullptr;
    void * lib = dlopen(info.dli_fname, RTLD_LAZY | RTLD_NOLOAD);
    return lib ? (mi_get_type_traits_t) dlsym(lib, "ggml_internal_get_type_traits") : nullptr;
}

// once per process: the weight-type table agrees with the ggml it runs under
static bool check_type_table() {
    const mi_get_type_traits_t traits = bound_type_traits();
    for (const mi_type_info & t : kMiTypes) {
        const ggml_type gt = (ggml_type) t.type;
        MI_ASSERT(ggml_blck_size(gt) == t.blck && ggml_type_size(gt) == (size_t) t.bytes);
        if (traits)
            MI_ASSERT(traits(gt).vec_dot_type == (t.act == MI_ACT_NONE ? GGML_TYPE_F32 : (ggml_type) mi_act_type(t.act)));
    }
    for (const mi_act_quant q : {MI_ACT_Q8_0, MI_ACT_Q8_1, MI_ACT_Q8_K}) {
        const ggml_type gt = (ggml_type) mi_act_type(q);
        MI_ASSERT(ggml_blck_size(gt) == mi_act_block(q) && ggml_type_size(gt) == (size_t) mi_act_block_bytes(q));
    }
    return true;
}

extern "C" {

bool ggml_backend_is_mi355x(ggml_backend_t backend) {
    return backend != nullptr && ggml_guid_matches(backend->guid, mi_guid());
}

ggml_backend_t ggml_backend_mi355x_init(int device) {
    if (device < 0 || device >= device_count()) {
        fprintf(stderr, "%s: invalid device %d (have %d)\n", __func__, device, device_count());
        return nullptr;
    }
    static const bool table_checked = check_type_table();
    (void) table_checked;
    auto * ctx = new mi_backend_ctx();
    ctx->device = device;
    ctx->name = "MI355X" + std::to_string(device);
    {
        mi_device_guard g(device);
        MI_CHECK(hipStreamCreate(&ctx->stream));
        op_tables(ctx);
    }
    auto * backend = new ggml_backend{mi_guid(), k_mi_backend_i, ctx};
    return backend;
}

void * ggml_backend_mi355x_get_stream(ggml_backend_t backend) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    return ((mi_backend_ctx *) backend->context)->stream;
}

int ggml_backend_mi355x_last_launch_count(ggml_backend_t backend) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    return ((mi_backend_ctx *) backend->context)->last_launches;
}

const char * ggml_backend_mi355x_last_mul_mat_route(ggml_backend_t backend) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    return g_mi_last_route;
}

void ggml_backend_mi355x_set_graph_capture(ggml_backend_t backend, bool enable) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    auto * ctx = (mi_backend_ctx *) backend->context;
    ctx->graphs = enable;
    ctx->graph_fail_streak = 0;
    ctx->topo_misses.clear();  // topologies switched to direct launch get captured again
}

void ggml_backend_mi355x_set_perf(ggml_backend_t backend, bool enable) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    ((mi_backend_ctx *) backend->context)->perf = enable;
}

void ggml_backend_mi355x_graph_stats(ggml_backend_t backend, int64_t * stats4) {
    ggml_backend_mi355x_graph_stats_ex(backend, stats4, 4);
}

int ggml_backend_mi355x_graph_stats_ex(ggml_backend_t backend, int64_t * stats, int n) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    const auto * ctx = (const mi_backend_ctx *) backend->context;
    const int m = std::min(n, (int) (sizeof(ctx->graph_stats) / sizeof(ctx->graph_stats[0])));
    for (int i = 0; i < m; i++) stats[i] = ctx->graph_stats[i];
    return m;
}

bool ggml_backend_mi355x_set_tuning(const char * name, int value) { return mi_tuning_set(name, value); }

size_t ggml_backend_mi355x_planes_stats(size_t * bytes) {
    if (bytes) *bytes = mi_planes_bytes();
    return mi_planes_count();
}

bool ggml_backend_mi355x_quantize_activations(ggml_backend_t backend, int vec_dot_type, const float * x, int64_t K,
                                              int64_t ncols, int8_t * qs, float * d, int16_t * s32) {
    MI_ASSERT(ggml_backend_is_mi355x(backend));
    const mi_act_quant q = q8_quant_of((ggml_type) vec_dot_type);
    const bool is_k = q == MI_ACT_Q8_K;
    const bool is_1 = q == MI_ACT_Q8_1;  // s32: the fp16 bits of the blocks' s
    if (q == MI_ACT_NONE || K % mi_act_block(q) != 0) return false;
    auto * ctx = (mi_backend_ctx *) backend->context;
    mi_device_guard g(ctx->device);
    const size_t xbytes = (size_t) K * ncols * sizeof(float);
    void * dx = nullptr;
    void * dq = nullptr;
    MI_CHECK(hipMalloc(&dx, xbytes));
    MI_CHECK(hipMalloc(&dq, mi_act_q8_bytes(K, ncols, q)));
    MI_CHECK(hipMemcpy(dx, x, xbytes, hipMemcpyHostToDevice));
    mi_src_cols src;
    src.base = (const char *) dx;
    src.ne1 = ncols;
    src.ne2 = src.ne3 = 1;
    src.nb1 = (size_t) K * sizeof(float);
    src.nb2 = src.nb3 = src.nb1 * ncols;
    const mi_act_q8 act = mi_act_q8_carve(dq, K, ncols, q);
    if (is_k) mi_quantize_q8_K(src, K, act, ctx->stream);
    else if (is_1) mi_quantize_q8_1(src, K, act, ctx->stream);
    else mi_quantize_q8_0(src, K, act, ctx->stream);
    MI_CHECK(hipStreamSynchronize(ctx->stream));
    MI_CHECK(hipMemcpy(qs, act.qs, (size_t) K * ncols, hipMemcpyDeviceToHost));
    MI_CHECK(hipMemcpy(d, act.d, (size_t) (K / mi_act_block(q)) * ncols * sizeof(float), hipMemcpyDeviceToHost));
    if ((is_k || is_1) && s32) MI_CHECK(hipMemcpy(s32, act.s32, (size_t) (K / 32) * ncols * sizeof(int16_t), hipMemcpyDeviceToHost));
    MI_CHECK(hipFree(dx));
    MI_CHECK(hipFree(dq));
    return true;
}

static ggml_backend_t mi_reg_init(const char * params, void * user_data) {
    (void) params;
    return ggml_backend_mi355x_init((int) (intptr_t) user_data);
}

int ggml_backend_mi355x_reg_devices(void) {
    static int registered = -1;
    if (registered >= 0) return registered;
    const int n = device_count();
    for (int i = 0; i < n; i++) {
        char name[128];
        snprintf(name, sizeof(name), "MI355X%d", i);
        ggml_backend_register(name, mi_reg_init, ggml_backend_mi355x_buffer_type(i), (void *) (intptr_t) i);
    }
    registered = n;
    return n;
}

} // extern "C"

// Plugging into the reference libggml (whose registry only knows the backends compiled into
// it, ggml-backend.c:417-450): with GGML_MI355X_AUTOREGISTER=1 the library registers its
// devices when loaded (e.g. LD_PRELOAD into the unmodified test-backend-ops). The reference
// registers its CPU entry on the first ggml_backend_reg_get_count() call, which keeps CPU at
// index 0 as there. The repo's own runtime instead looks this library up lazily on its first
// registry query (csrc/core/ggml_backend_rt.cpp), so loading it never touches the GPU.
__attribute__((constructor)) static void mi_autoregister(void) {
    if (env_int("GGML_MI355X_AUTOREGISTER", 0) == 0) return;
    (void) ggml_backend_reg_get_count();
    ggml_backend_mi355x_reg_devices();
}
