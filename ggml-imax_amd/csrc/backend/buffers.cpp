// buffers.cpp -- the MI355X backend's devices, its three buffer types (device, pinned host,
// tensor-split rows) and their buffers, with the buffer-type entry points of the public API.
// Structural analogue in the reference: src/ggml-cuda.cu:366-576 (buffers, buffer types), :578-975
// (split buffers), :979-1050 (host buffers).

#include "mi_backend.h"

#include <map>
#include <mutex>

// ---------------------------------------------------------------------------------------------
// devices
// ---------------------------------------------------------------------------------------------

int device_count() {
    static int count = [] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        return std::min(n, GGML_MI355X_MAX_DEVICES);
    }();
    return count;
}

// ---------------------------------------------------------------------------------------------
// device buffer
// ---------------------------------------------------------------------------------------------

static const char * mi_buffer_get_name(ggml_backend_buffer_t buffer) {
    return ((mi_buffer_ctx *) buffer->context)->name.c_str();
}

bool buffer_is_mi355x(ggml_backend_buffer_t buffer) {
    return buffer && buffer->iface.get_name == mi_buffer_get_name;
}

static void mi_buffer_free(ggml_backend_buffer_t buffer) {
    auto * ctx = (mi_buffer_ctx *) buffer->context;
    mi_device_guard g(ctx->device);
    mi_planes_drop(ctx->dev_ptr, buffer->size);
    MI_CHECK(hipFree(ctx->dev_ptr));
    delete ctx;
}

static void * mi_buffer_get_base(ggml_backend_buffer_t buffer) { return ((mi_buffer_ctx *) buffer->context)->dev_ptr; }

static void mi_buffer_set_tensor(ggml_backend_buffer_t buffer, ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    auto * ctx = (mi_buffer_ctx *) buffer->context;
    mi_device_guard g(ctx->device);
    // null stream: ordered after any queued work on the (blocking) backend streams
    MI_CHECK(hipMemcpyAsync((char *) tensor->data + offset, data, size, hipMemcpyHostToDevice, nullptr));
    mi_planes_refresh((char *) tensor->data + offset, size, nullptr);  // repacked planes over these bytes
    MI_CHECK(hipStreamSynchronize(nullptr));
}

static void mi_buffer_get_tensor(ggml_backend_buffer_t buffer, const ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    auto * ctx = (mi_buffer_ctx *) buffer->context;
    mi_device_guard g(ctx->device);
    MI_CHECK(hipMemcpyAsync(data, (const char *) tensor->data + offset, size, hipMemcpyDeviceToHost, nullptr));
    MI_CHECK(hipStreamSynchronize(nullptr));
}

static bool mi_buffer_cpy_tensor(ggml_backend_buffer_t buffer, const ggml_tensor * src, ggml_tensor * dst) {
    ggml_backend_buffer_t src_buf = src->view_src ? src->view_src->buffer : src->buffer;
    if (!buffer_is_mi355x(src_buf)) return false;
    auto * sctx = (mi_buffer_ctx *) src_buf->context;
    auto * dctx = (mi_buffer_ctx *) buffer->context;
    mi_device_guard g(dctx->device);
    if (sctx->device == dctx->device) {
        MI_CHECK(hipMemcpyAsync(dst->data, src->data, ggml_nbytes(src), hipMemcpyDeviceToDevice, nullptr));
    } else {
        MI_CHECK(hipMemcpyPeerAsync(dst->data, dctx->device, src->data, sctx->device, ggml_nbytes(src), nullptr));
    }
    mi_planes_refresh(dst->data, ggml_nbytes(src), nullptr);
    MI_CHECK(hipStreamSynchronize(nullptr));
    return true;
}

static void mi_buffer_clear(ggml_backend_buffer_t buffer, uint8_t value) {
    auto * ctx = (mi_buffer_ctx *) buffer->context;
    mi_device_guard g(ctx->device);
    MI_CHECK(hipMemset(ctx->dev_ptr, value, buffer->size));
    mi_planes_refresh(ctx->dev_ptr, buffer->size, nullptr);
    MI_CHECK(hipStreamSynchronize(nullptr));
}

static const ggml_backend_buffer_i k_mi_buffer_i = {
    /* get_name    */ mi_buffer_get_name,
    /* free_buffer */ mi_buffer_free,
    /* get_base    */ mi_buffer_get_base,
    /* init_tensor */ nullptr,
    /* set_tensor  */ mi_buffer_set_tensor,
    /* get_tensor  */ mi_buffer_get_tensor,
    /* cpy_tensor  */ mi_buffer_cpy_tensor,
    /* clear       */ mi_buffer_clear,
    /* reset       */ nullptr,
};

// ---------------------------------------------------------------------------------------------
// device buffer type (one static instance per device, ggml-cuda.cu:553-576)
// ---------------------------------------------------------------------------------------------

struct mi_buft_ctx {
    int device;
    std::string name;
};

static const char * mi_buft_get_name(ggml_backend_buffer_type_t buft) { return ((mi_buft_ctx *) buft->context)->name.c_str(); }

static ggml_backend_buffer_t mi_buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    auto * bctx = (mi_buft_ctx *) buft->context;
    mi_device_guard g(bctx->device);
    size = std::max(size, (size_t) 1);
    void * ptr = nullptr;
    const hipError_t err = hipMalloc(&ptr, size + kBufferSlack);
    if (err != hipSuccess) {
        (void) hipGetLastError();
        fprintf(stderr, "%s: allocating %.2f MiB on device %d: hipMalloc failed: %s\n", __func__,
                size / 1024.0 / 1024.0, bctx->device, hipGetErrorString(err));
        return nullptr;
    }
    auto * ctx = new mi_buffer_ctx{bctx->device, ptr, "MI355X" + std::to_string(bctx->device)};
    return ggml_backend_buffer_init(buft, k_mi_buffer_i, ctx, size);
}

static size_t mi_buft_get_alignment(ggml_backend_buffer_type_t) { return kBufferAlign; }

static size_t mi_buft_get_max_size(ggml_backend_buffer_type_t) { return SIZE_MAX; }

static size_t mi_buft_get_alloc_size(ggml_backend_buffer_type_t, const ggml_tensor * tensor) { return ggml_nbytes(tensor); }

static bool mi_buft_supports_backend(ggml_backend_buffer_type_t buft, ggml_backend_t backend);

static const ggml_backend_buffer_type_i k_mi_buft_i = {
    /* get_name         */ mi_buft_get_name,
    /* alloc_buffer     */ mi_buft_alloc_buffer,
    /* get_alignment    */ mi_buft_get_alignment,
    /* get_max_size     */ mi_buft_get_max_size,
    /* get_alloc_size   */ mi_buft_get_alloc_size,
    /* supports_backend */ mi_buft_supports_backend,
    /* is_host          */ nullptr,
};

// ---------------------------------------------------------------------------------------------
// pinned host buffer type (ggml-cuda.cu:979-1050)
// ---------------------------------------------------------------------------------------------

static const char * mi_host_buffer_name(ggml_backend_buffer_t) { return "MI355X_Host"; }
static void mi_host_buffer_free(ggml_backend_buffer_t b) { MI_CHECK(hipHostFree(b->context)); }
static void * mi_host_buffer_base(ggml_backend_buffer_t b) { return b->context; }
static void mi_host_buffer_set(ggml_backend_buffer_t, ggml_tensor * t, const void * d, size_t o, size_t n) { memcpy((char *) t->data + o, d, n); }
static void mi_host_buffer_get(ggml_backend_buffer_t, const ggml_tensor * t, void * d, size_t o, size_t n) { memcpy(d, (const char *) t->data + o, n); }
static void mi_host_buffer_clear(ggml_backend_buffer_t b, uint8_t v) { memset(b->context, v, b->size); }

static const ggml_backend_buffer_i k_mi_host_buffer_i = {
    mi_host_buffer_name, mi_host_buffer_free, mi_host_buffer_base, nullptr, mi_host_buffer_set, mi_host_buffer_get,
    nullptr, mi_host_buffer_clear, nullptr,
};

static const char * mi_host_buft_name(ggml_backend_buffer_type_t) { return "MI355X_Host"; }

static ggml_backend_buffer_t mi_host_buft_alloc(ggml_backend_buffer_type_t buft, size_t size) {
    void * ptr = nullptr;
    if (hipHostMalloc(&ptr, std::max(size, (size_t) 1), hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) {
        (void) hipGetLastError();
        // fall back to pageable host memory of the runtime's host buffer type
        return ggml_backend_buft_alloc_buffer(ggml_backend_cpu_buffer_type(), size);
    }
    return ggml_backend_buffer_init(buft, k_mi_host_buffer_i, ptr, size);
}

static size_t mi_host_buft_align(ggml_backend_buffer_type_t) { return 64; }
// pinned host memory is ordinary CPU memory to the scheduler: whatever backend can use a CPU
// buffer can use this one (ggml-cuda.cu:1037-1038 delegates the same way)
static bool mi_host_buft_supports(ggml_backend_buffer_type_t, ggml_backend_t backend) {
    ggml_backend_buffer_type_t cpu = ggml_backend_cpu_buffer_type();
    return cpu->iface.supports_backend(cpu, backend);
}
static bool mi_host_buft_is_host(ggml_backend_buffer_type_t) { return true; }

// ---------------------------------------------------------------------------------------------
// tensor-split row buffer type (ggml-cuda.cu:578-975 analogue)
// ---------------------------------------------------------------------------------------------
// The rows of each weight matrix are divided over "slots" by the cumulative fractions given to
// ggml_backend_mi355x_split_buffer_type(); slot s lives on device s. With the test setting
// GGML_MI355X_SPLIT_SLOTS=n on a machine with fewer devices, slot s lives on device s % count,
// still with its own allocation, stream and copies, so the whole multi-device path (activation
// copy in, per-slot GEMM, gather of the row slices) runs on one GPU. GGML_OP_MUL_MAT with such a
// weight is op_mul_mat_split (mul_mat.cpp).

int split_slots() {
    static int n = [] {
        const int v = mi_env_split_slots();
        return v > 0 ? std::min(v, GGML_MI355X_MAX_DEVICES) : std::max(device_count(), 1);
    }();
    return n;
}

int slot_device(int slot) { return slot % std::max(device_count(), 1); }

struct mi_split_buft_ctx {
    std::vector<float> split;  // cumulative start fraction of each slot
};
struct mi_split_buffer_ctx {
    std::vector<mi_split_extra *> extras;
};

// slices start on multiples of the GEMM's 64-row tile (any row count is valid for every kernel)
static constexpr int64_t kSplitRowRounding = 64;

static void split_rows(const ggml_tensor * t, const mi_split_buft_ctx * c, int slot, int64_t & lo, int64_t & hi) {
    const int64_t nrows = ggml_nrows(t);
    const int n = (int) c->split.size();
    lo = slot == 0 ? 0 : (int64_t) ((double) nrows * c->split[slot]);
    lo -= lo % kSplitRowRounding;
    if (slot == n - 1) {
        hi = nrows;
    } else {
        hi = (int64_t) ((double) nrows * c->split[slot + 1]);
        hi -= hi % kSplitRowRounding;
    }
    hi = std::max(hi, lo);
}

static const char * mi_split_buffer_name(ggml_backend_buffer_t) { return "MI355X_Split"; }

static bool buffer_is_split(ggml_backend_buffer_t buffer) {
    return buffer && buffer->iface.get_name == mi_split_buffer_name;
}

bool is_split_tensor(const ggml_tensor * t) {
    const ggml_tensor * base = t->view_src ? t->view_src : t;
    return buffer_is_split(base->buffer);
}

static void mi_split_buffer_free(ggml_backend_buffer_t buffer) {
    auto * ctx = (mi_split_buffer_ctx *) buffer->context;
    for (mi_split_extra * e : ctx->extras) {
        for (const auto & sl : e->slices) {
            mi_device_guard g(sl.device);
            MI_CHECK(hipFree(sl.ptr));
        }
        delete e;
    }
    delete ctx;
}

static void * mi_split_buffer_base(ggml_backend_buffer_t) {
    return (void *) 0x1000;  // the slices' pointers live in tensor->extra; never dereferenced
}

static void mi_split_buffer_init_tensor(ggml_backend_buffer_t buffer, ggml_tensor * tensor) {
    MI_ASSERT(tensor->view_src == nullptr && "views of split tensors are not supported");
    auto * ctx = (mi_split_buffer_ctx *) buffer->context;
    auto * bctx = (mi_split_buft_ctx *) buffer->buft->context;
    auto * extra = new mi_split_extra();
    ctx->extras.push_back(extra);
    const size_t nb1 = ggml_row_size(tensor->type, tensor->ne[0]);
    for (int s = 0; s < (int) bctx->split.size(); s++) {
        int64_t lo, hi;
        split_rows(tensor, bctx, s, lo, hi);
        if (hi == lo) continue;
        mi_split_slice sl{s, slot_device(s), lo, hi, nullptr};
        mi_device_guard g(sl.device);
        const size_t bytes = (size_t) (hi - lo) * nb1;
        MI_CHECK(hipMalloc((void **) &sl.ptr, bytes + kBufferSlack));  // init_tensor cannot fail (ggml-cuda.cu:755)
        MI_CHECK(hipMemset(sl.ptr + bytes, 0, kBufferSlack));
        extra->slices.push_back(sl);
    }
    tensor->extra = extra;
}

static void mi_split_buffer_set_tensor(ggml_backend_buffer_t, ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    // split tensors are set whole (ggml-cuda.cu:781-782)
    MI_ASSERT(offset == 0 && size == ggml_nbytes(tensor));
    const auto * extra = (const mi_split_extra *) tensor->extra;
    for (const auto & sl : extra->slices) {
        mi_device_guard g(sl.device);
        MI_CHECK(hipMemcpy(sl.ptr, (const char *) data + sl.row_low * tensor->nb[1], (size_t) (sl.row_high - sl.row_low) * tensor->nb[1],
                           hipMemcpyHostToDevice));
    }
}

static void mi_split_buffer_get_tensor(ggml_backend_buffer_t, const ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    MI_ASSERT(offset == 0 && size == ggml_nbytes(tensor));
    const auto * extra = (const mi_split_extra *) tensor->extra;
    for (const auto & sl : extra->slices) {
        mi_device_guard g(sl.device);
        MI_CHECK(hipMemcpy((char *) data + sl.row_low * tensor->nb[1], sl.ptr, (size_t) (sl.row_high - sl.row_low) * tensor->nb[1],
                           hipMemcpyDeviceToHost));
    }
}

static void mi_split_buffer_clear(ggml_backend_buffer_t, uint8_t) {}  // as ggml-cuda.cu:856-859

static const ggml_backend_buffer_i k_mi_split_buffer_i = {
    /* get_name    */ mi_split_buffer_name,
    /* free_buffer */ mi_split_buffer_free,
    /* get_base    */ mi_split_buffer_base,
    /* init_tensor */ mi_split_buffer_init_tensor,
    /* set_tensor  */ mi_split_buffer_set_tensor,
    /* get_tensor  */ mi_split_buffer_get_tensor,
    /* cpy_tensor  */ nullptr,
    /* clear       */ mi_split_buffer_clear,
    /* reset       */ nullptr,
};

static const char * mi_split_buft_name(ggml_backend_buffer_type_t) { return "MI355X_Split"; }

static ggml_backend_buffer_t mi_split_buft_alloc(ggml_backend_buffer_type_t buft, size_t size) {
    // the slices are allocated per tensor in init_tensor, once the rounded split is known; size is
    // the bound ggml-alloc enforces with get_alloc_size (ggml-cuda.cu:887-895)
    return ggml_backend_buffer_init(buft, k_mi_split_buffer_i, new mi_split_buffer_ctx(), size);
}

static size_t mi_split_buft_align(ggml_backend_buffer_type_t) { return kBufferAlign; }

static size_t mi_split_buft_alloc_size(ggml_backend_buffer_type_t buft, const ggml_tensor * tensor) {
    auto * c = (mi_split_buft_ctx *) buft->context;
    const size_t nb1 = ggml_row_size(tensor->type, tensor->ne[0]);
    size_t total = 0;
    for (int s = 0; s < (int) c->split.size(); s++) {
        int64_t lo, hi;
        split_rows(tensor, c, s, lo, hi);
        if (hi > lo) total += (size_t) (hi - lo) * nb1 + kBufferSlack;
    }
    return std::max(total, ggml_nbytes(tensor));
}

static bool mi_split_buft_supports(ggml_backend_buffer_type_t, ggml_backend_t backend) { return ggml_backend_is_mi355x(backend); }

static const ggml_backend_buffer_type_i k_mi_split_buft_i = {
    /* get_name         */ mi_split_buft_name,
    /* alloc_buffer     */ mi_split_buft_alloc,
    /* get_alignment    */ mi_split_buft_align,
    /* get_max_size     */ nullptr,
    /* get_alloc_size   */ mi_split_buft_alloc_size,
    /* supports_backend */ mi_split_buft_supports,
    /* is_host          */ nullptr,
};

static bool mi_buft_supports_backend(ggml_backend_buffer_type_t buft, ggml_backend_t backend) {
    if (!ggml_backend_is_mi355x(backend)) return false;
    return ((mi_buft_ctx *) buft->context)->device == ((mi_backend_ctx *) backend->context)->device;
}

// ---- public API: the buffer types ----------------------------------------------------------

extern "C" {

ggml_backend_buffer_type_t ggml_backend_mi355x_buffer_type(int device) {
    static std::mutex mutex;
    static ggml_backend_buffer_type types[GGML_MI355X_MAX_DEVICES];
    static mi_buft_ctx ctxs[GGML_MI355X_MAX_DEVICES];
    static bool initialized = false;
    std::lock_guard<std::mutex> lock(mutex);
    if (device < 0 || device >= device_count()) return nullptr;
    if (!initialized) {
        for (int i = 0; i < GGML_MI355X_MAX_DEVICES; i++) {
            ctxs[i] = mi_buft_ctx{i, "MI355X" + std::to_string(i)};
            types[i] = ggml_backend_buffer_type{k_mi_buft_i, &ctxs[i]};
        }
        initialized = true;
    }
    return &types[device];
}

ggml_backend_buffer_type_t ggml_backend_mi355x_host_buffer_type(void) {
    static ggml_backend_buffer_type buft = {
        {mi_host_buft_name, mi_host_buft_alloc, mi_host_buft_align, nullptr, nullptr, mi_host_buft_supports, mi_host_buft_is_host},
        nullptr,
    };
    return &buft;
}

ggml_backend_buffer_type_t ggml_backend_mi355x_split_buffer_type(const float * tensor_split) {
    // one buffer type per distinct split, kept for the process lifetime (ggml-cuda.cu:941-975);
    // tensor_split: GGML_MI355X_MAX_DEVICES proportions (all zero / null = equal rows per slot)
    static std::mutex mutex;
    static std::map<std::vector<float>, ggml_backend_buffer_type *> types;
    std::lock_guard<std::mutex> lock(mutex);
    const int n = split_slots();
    std::vector<float> cum(n, 0.0f);
    const bool all_zero = tensor_split == nullptr || std::all_of(tensor_split, tensor_split + n, [](float v) { return v == 0.0f; });
    float sum = 0.0f;
    for (int i = 0; i < n; i++) {
        cum[i] = sum;
        sum += all_zero ? 1.0f : std::max(tensor_split[i], 0.0f);
    }
    for (int i = 0; i < n; i++) cum[i] /= sum;
    auto it = types.find(cum);
    if (it != types.end()) return it->second;
    auto * buft = new ggml_backend_buffer_type{k_mi_split_buft_i, new mi_split_buft_ctx{cum}};
    types.emplace(cum, buft);
    return buft;
}

} // extern "C"
