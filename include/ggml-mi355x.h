// ggml-mi355x.h -- C-ABI entry points of the MI355X (gfx950) ggml backend.
//
// Drop-in counterpart of the reference's device-backend header src/ggml-cuda.h:19-40
// (NAIST-Archlab/ggml-imax @ v2); each function cites the declaration it replaces. Everything
// else a caller needs goes through the generic ggml_backend_* API (include/ggml_abi.h), exactly
// as with the CUDA and Metal backends. The library also registers one registry entry per
// device ("MI355X0", "MI355X1", ...) from an ELF constructor, so registry-driven tools
// (tests/test-backend-ops.cpp, ggml_backend_reg_init_backend_from_str) find it unmodified.
#pragma once

#include "ggml_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GGML_MI355X_MAX_DEVICES 16

// ggml-cuda.h:21  ggml_backend_cuda_init(int device)
GGML_API ggml_backend_t ggml_backend_mi355x_init(int device);

// ggml-cuda.h:23  ggml_backend_is_cuda(ggml_backend_t)
GGML_API bool ggml_backend_is_mi355x(ggml_backend_t backend);

// ggml-cuda.h:26  ggml_backend_cuda_buffer_type(int device): device-resident (HBM) buffers
GGML_API ggml_backend_buffer_type_t ggml_backend_mi355x_buffer_type(int device);

// ggml-cuda.h:29  ggml_backend_cuda_split_buffer_type(const float * tensor_split): rows of a
// matrix split across devices (tensor-split row path); tensor_split = GGML_MI355X_MAX_DEVICES
// proportions (NULL / all zero = equal), slices rounded to 64-row GEMM tiles
GGML_API ggml_backend_buffer_type_t ggml_backend_mi355x_split_buffer_type(const float * tensor_split);

// ggml-cuda.h:32  ggml_backend_cuda_host_buffer_type(): pinned host memory for fast H2D/D2H
GGML_API ggml_backend_buffer_type_t ggml_backend_mi355x_host_buffer_type(void);

// ggml-cuda.h:34-36
GGML_API int  ggml_backend_mi355x_get_device_count(void);
GGML_API void ggml_backend_mi355x_get_device_description(int device, char * description, size_t description_size);
GGML_API void ggml_backend_mi355x_get_device_memory(int device, size_t * free, size_t * total);

// ggml-cuda.h:38-39
GGML_API bool ggml_backend_mi355x_register_host_buffer(void * buffer, size_t size);
GGML_API void ggml_backend_mi355x_unregister_host_buffer(void * buffer);

// ggml-cuda.cu:3024-3042 ggml_backend_cuda_reg_devices (called by the reference registry init;
// here also run from the library constructor). Returns the number of devices registered.
GGML_API int ggml_backend_mi355x_reg_devices(void);

// --- MI355X extensions (no reference counterpart) ---

// hipStream_t the backend launches on (for external timing with HIP events / stream interop)
GGML_API void * ggml_backend_mi355x_get_stream(ggml_backend_t backend);

// Number of kernels launched by the last graph_compute (for tests / profiling).
GGML_API int ggml_backend_mi355x_last_launch_count(ggml_backend_t backend);

// The kernel the launchers picked for the most recent quantized or F16 MUL_MAT / MUL_MAT_ID launch from
// the host (a replayed capture launches none): a string that stays valid, such as "k_mmqp", "k_mmqt",
// "k_mmv_kq_ord<nc8>", "k_mmv_stream<type12,nc1,pd3,...>", and for F16 weights
// "k_gemv_f16<nc4,u2,one,jm0,epi1,xh0>[ks3,rgs1]", "k_gemv_f16_bn<nw16,ks4,epi3>", "k_gemv_f16_ps<npm12,qpt1,epi3>[rw4]",
// "k_gemv_f16_tall<nc8,u8,jm4,epi1>", "k_gemv_f16_mt<jm0,nk24,epi0>", "k_mmv_f16_w16<nc1,ks48,epi0>[t256]",
// "k_mmv_f16_x<nc1,u32,epi0>[t64]", "k_mmv_f16_ord<nc4,aligned1,id0>", "k_mmf16p<pf3>", "k_mmq3<sk2,nst16>": the
// template arguments that select an instance, then in square brackets the launch geometry a knob moves.
// "" before the first. For tests: a forced route (set_tuning) that the shape makes the launcher ignore shows here.
GGML_API const char * ggml_backend_mi355x_last_mul_mat_route(ggml_backend_t backend);

// hipGraphs. graph_compute captures a graph's launches and replays the capture whenever the same
// graph (same nodes, addresses, shapes, parameters) is computed again, updating an executable
// graph of the same topology in place when only kernel arguments changed (the reference's CUDA
// graphs, ggml-cuda.cu:2456-2713); the first graph of a topology, and graphs of fewer than 4
// kernel launches (GGML_MI355X_GRAPH_MIN_LAUNCHES), launch directly. Graph plans
// (ggml_backend_graph_plan_create / _compute) are captured at creation and computed with one
// hipGraphLaunch. GGML_MI355X_DISABLE_GRAPHS=1 (process-wide, as GGML_CUDA_DISABLE_GRAPHS,
// ggml-cuda.cu:2462) or set_graph_capture(false) makes both launch directly.
GGML_API void ggml_backend_mi355x_set_graph_capture(ggml_backend_t backend, bool enable);
// Per-node timer, the reference's GGML_PERF (ggml.c:19195-19205, :19907-19922) for this backend:
// with it on (or GGML_MI355X_PERF set), graphs launch directly and every node's device time is
// measured with HIP events around the kernel that computes it; node->perf_runs / perf_time_us (and
// perf_cycles, in microseconds) and the cgraph's totals accumulate as the reference's CPU executor
// fills them, and ggml_graph_print() prints them. A fused chain's time goes to its last node, the
// others get runs without time. Timing synchronizes the stream once per graph.
GGML_API void ggml_backend_mi355x_set_perf(ggml_backend_t backend, bool enable);
// counters since init: [0] captures (plans and graph_compute), [1] graph instantiations,
// [2] in-place updates, [3] direct (uncaptured) computes
GGML_API void ggml_backend_mi355x_graph_stats(ggml_backend_t backend, int64_t * stats4);
// the same counters and more: [4] graph_compute replays of a cached capture, [5] graph_compute
// captures; fills min(n, available) entries and returns that count
GGML_API int ggml_backend_mi355x_graph_stats_ex(ggml_backend_t backend, int64_t * stats, int n);

// Launch-shape knobs of the kernels, for A/B tuning inside one process: "mmv_blocks" (resident
// workgroups of the fused GEMV), "mmv_variant", ... (the fields of mi_tuning, mi355x_kernels.h).
// GGML_MI355X_<NAME>=value in the environment sets the same knob at start-up, with the same range
// check. Returns false for an unknown name or a value the knob does not accept.
GGML_API bool ggml_backend_mi355x_set_tuning(const char * name, int value);

// Runs the device activation quantizer that GGML_OP_MUL_MAT uses for `vec_dot_type`
// (GGML_TYPE_Q8_0, GGML_TYPE_Q8_1 or GGML_TYPE_Q8_K) on ncols host columns of K floats and returns
// its structure-of-arrays result: qs [ncols*K], d [ncols*K/QK], s32 [ncols*K/32] (Q8_K: sums of 32
// quants; Q8_1: the fp16 bits of each block's s). Lets tests compare the device rounding with the
// reference bit for bit.
GGML_API bool ggml_backend_mi355x_quantize_activations(ggml_backend_t backend, int vec_dot_type, const float * x,
                                                       int64_t K, int64_t ncols, int8_t * qs, float * d, int16_t * s32);

// Repacked MFMA planes of Q4_K / Q5_K weights kept for long prompts (no reference counterpart: the
// reference's CPU mul_mat dequantizes per call): how many weight tensors carry them, and their bytes
GGML_API size_t ggml_backend_mi355x_planes_stats(size_t * bytes);

#ifdef __cplusplus
}
#endif
