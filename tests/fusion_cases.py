"""Small graphs around the backend's fusion passes (csrc/backend/fusion.cpp: try_fuse_norm, try_fuse_softmax,
collect_epilogue / try_fuse_f16_gemv / try_fuse_q_gemv, try_fuse_copies, try_fuse_embedding, plan_attention,
try_fuse_attn_proj), shared by tests/test_fusion.py (reference CPU alone) and tests/test_fusion_gpu.py.

A case is a graph `build(L, c) -> (feeds, outs)` through any library exporting the ggml API. `outs` maps a
name to a tensor, expanded into the graph in that order: the final value, named "out", and every intermediate
the graph semantically materialises because it has a second reader or is flagged output. A *positive* case is
a pattern its pass absorbs: `absorbed` is the number of nodes that then get no launch of their own, so the
backend launches (non-noop nodes - absorbed) kernels. A *near-miss* case breaks one legality condition of a
pass (or is legal but sits on a guard's edge): only its values are pinned. The epilogue/aliased cases are
refusals whose launch count is known and asserted like a positive case's.

Inputs come from synth.uniform. Every operand a fusion could wrongly absorb or drop (`absorbable`: operand ->
output it must move) is scaled so that leaving it out moves that output by at least 100 x the tolerance of the
comparison; tests/test_fusion.py checks that on the reference CPU by zeroing the operand (scale: set to 1).

Tolerances in tree order (mmv_order 0), relative to max |ref|, all the project's existing ones; with
mmv_order 1 every output is the reference CPU's bits.
"""
import ctypes

import numpy as np

from ggml_mi355x import ggml as G
from ggml_mi355x import synth
from weight_types import TREE_TOL, quantize

F32, F16, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32
Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = G.GGML_TYPE_Q4_0, G.GGML_TYPE_Q8_0, G.GGML_TYPE_Q4_K, G.GGML_TYPE_Q5_K, G.GGML_TYPE_Q6_K
TYPE_NAME = {F16: "f16", Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K"}

EXACT = 0.0
TOL_Q = TREE_TOL   # quantized GEMV outputs (weight_types.py)
TOL_F16 = 1e-3     # F16 GEMV outputs (test_norm_prologue_gemv_columns)
TOL_GELU = 2e-4    # outputs behind a fused GELU (test_attention_projection_fused)
TOL_ATTN = 5e-5    # tree-order attention (test_gpt2_attention_block_exact)

GGML_TENSOR_FLAG_OUTPUT = 2
NOOP_OPS = {"NONE", "RESHAPE", "VIEW", "PERMUTE", "TRANSPOSE"}
LONG_ROW = 12290   # k_norm / k_soft_max stage rows longer than 12288 floats in dst
N_OUT = 96         # rows of every weight matrix


def u(seed, n, scale=1.0, shift=0.0):
    return (synth.uniform(seed, int(n)) * np.float32(scale) + np.float32(shift)).astype(np.float32)


def new(L, c, ttype, *ne):
    return getattr(L, f"ggml_new_tensor_{len(ne)}d")(c, ttype, *ne)


def op_name(L, t):
    return L.ggml_op_name(t.contents.op).decode()


def _bind(L, name, argtypes):
    """A reference-API function G._SIGS does not list, if the library exports it."""
    for h in L.handles:
        try:
            fn = getattr(h, name)
        except AttributeError:
            continue
        fn.argtypes, fn.restype = argtypes, G.T
        return fn
    return None


def _unary_of(a, like, op_from):
    """A node built by hand where the library has no builder for it: `like` (a tensor shaped as `a`, or a
    view of it) gets src[0] = a and the op and op_params of the node `op_from`."""
    like.contents.op = op_from.contents.op
    for k in range(16):
        like.contents.op_params[k] = op_from.contents.op_params[k]
    like.contents.src[0] = ctypes.cast(a, ctypes.c_void_p).value
    return like


def rms_norm_inplace(L, c, a, eps):
    fn = _bind(L, "ggml_rms_norm_inplace", [ctypes.c_void_p, G.T, ctypes.c_float])
    if fn:
        return fn(c, a, eps)
    view = _bind(L, "ggml_view_tensor", [ctypes.c_void_p, G.T])(c, a)
    return _unary_of(a, view, L.ggml_rms_norm(c, a, eps))


def diag_mask_zero(L, c, a, n_past):
    fn = _bind(L, "ggml_diag_mask_zero", [ctypes.c_void_p, G.T, ctypes.c_int])
    if fn:
        return fn(c, a, n_past)
    # the runtime's core implements the builders its GPT-2 / LLaMA drivers call, and none of them masks with zero:
    # the node is a DIAG_MASK_INF node with the next op code (the backend and supports_op do know the op)
    r = L.ggml_diag_mask_inf(c, a, n_past)
    r.contents.op += 1
    assert op_name(L, r) == "DIAG_MASK_ZERO"
    return r


def diag_mask_inf_inplace(L, c, a, n_past):
    return _bind(L, "ggml_diag_mask_inf_inplace", [ctypes.c_void_p, G.T, ctypes.c_int])(c, a, n_past)


def add_inplace(L, c, a, b):
    return _bind(L, "ggml_add_inplace", [ctypes.c_void_p, G.T, G.T])(c, a, b)


def flag_output(t):
    t.contents.flags |= GGML_TENSOR_FLAG_OUTPUT
    return t


_weights = {}


def weight_bytes(L, wtype, K, N, seed):
    key = (wtype, K, N, seed)
    if key not in _weights:
        w = u(seed, K * N, 0.05 if wtype == F16 else 1.0)
        _weights[key] = w.astype(np.float16) if wtype == F16 else quantize(L, wtype, w, K)
    return _weights[key]


class Builder:
    """What a case's graph function gets: the library, the context for compute tensors, the context for
    leaves (the same one unless the graph allocator lays out the compute tensors) and the feeds."""

    def __init__(self, L, c, case, leaves=None):
        self.L, self.c, self.case, self.lc = L, c, case, leaves if leaves is not None else c
        self.feeds = []
        self.first = []   # nodes expanded into the graph before `outs`, read by no test
        self.masks = {}   # out name -> bool array of the elements that are defined

    def leaf(self, name, arr, *ne, ttype=F32):
        t = new(self.L, self.lc, ttype, *ne)
        arr = np.asarray(arr)
        if self.case.drop == name:
            arr = np.zeros_like(arr)
        self.feeds.append((t, arr))
        if self.lc is not self.c and name in ("x", "cur", "resid") and ttype == F32:
            # under the graph allocator an input is a computed tensor (the same bits), so that its memory
            # is free for a later node's output once its last reader has run; these nodes come first in
            # the graph, ahead of the chain under test
            t = self.L.ggml_scale(self.c, t, 1.0)
            self.first.append(t)
        return t

    def weight(self, wtype, K, N, seed):
        t = new(self.L, self.lc, wtype, K, N)
        self.feeds.append((t, weight_bytes(self.L, wtype, K, N, seed)))
        return t

    def scale(self, v):
        return 1.0 if self.case.drop == "scale" else float(v)


class Case:
    def __init__(self, name, fn, positive, absorbed=0, tol=EXACT, absorbable=None, orders=(1, 0), n_tensors=96):
        self.name, self.fn, self.positive, self.orders, self.n_tensors = name, fn, positive, orders, n_tensors
        self._absorbed, self._tol = absorbed, tol
        self.absorbable = absorbable or {}
        self.drop = None
        self.masks = {}

    def absorbed(self, order):
        return self._absorbed[order] if isinstance(self._absorbed, dict) else self._absorbed

    def tol(self, out_name):
        """Bound on max |got - ref| / max |ref| in tree order; EXACT: identical bits."""
        return self._tol.get(out_name, EXACT) if isinstance(self._tol, dict) else self._tol

    def build(self, L, c, leaves=None):
        b = Builder(L, c, self, leaves)
        outs = self.fn(b)
        self.masks = b.masks
        return b.feeds, outs, b.first

    def __repr__(self):
        return self.name


CASES = []


def add(name, fn, positive, **kw):
    CASES.append(Case(name, fn, positive, **kw))


def by_prefix(prefix, positive=None):
    return [c for c in CASES if c.name.startswith(prefix) and (positive is None or c.positive == positive)]


# ------------------------------------------------------------------ running a case

def read(L, t):
    tt = t.contents.type
    return G.tensor_get(L, t, np.float16 if tt == F16 else (np.int32 if tt == I32 else np.float32))


def graph_nodes(g):
    gc = g.contents
    return [gc.nodes[i] for i in range(gc.n_nodes)]


def launch_nodes(L, g):
    """The nodes the backend launches something for when it fuses nothing."""
    return sum(1 for t in graph_nodes(g) if op_name(L, t) not in NOOP_OPS and L.ggml_nelements(t) > 0)


def run_case(L, backend, cs, drop=None, inspect=None):
    """Builds and computes `cs` with every tensor in storage of its own. Returns name -> values, the
    count of launch nodes, the backend's launch count (0 for a library without one) and inspect(L, graph)."""
    cs.drop = drop
    try:
        with G.Context(L, L.ggml_tensor_overhead() * cs.n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
            feeds, outs, first = cs.build(L, c.ctx)
            g = L.ggml_new_graph(c.ctx)
            for t in first + list(outs.values()):
                L.ggml_build_forward_expand(g, t)
            buf = L.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
            assert buf, "buffer allocation failed"
            try:
                for t, arr in feeds:
                    G.tensor_set(L, t, arr)
                seen = inspect(L, g) if inspect else None
                assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                n = L.ggml_backend_mi355x_last_launch_count(backend) if L.has("ggml_backend_mi355x_last_launch_count") else 0
                return {k: read(L, t) for k, t in outs.items()}, launch_nodes(L, g), n, seen
            finally:
                L.ggml_backend_buffer_free(buf)
    finally:
        cs.drop = None


def run_case_gallocr(L, backend, cs):
    """As test_moe_block_in_a_graph_allocator_buffer: leaves in a context and buffer of their own, compute
    tensors laid out by ggml_gallocr, which reuses the memory of dead tensors. Returns the final value, the
    backend's launch count and the compute buffer's size."""
    size = L.ggml_tensor_overhead() * cs.n_tensors + L.ggml_graph_overhead()
    with G.Context(L, size, no_alloc=True) as cl, G.Context(L, size, no_alloc=True) as c:
        feeds, outs, first = cs.build(L, c.ctx, leaves=cl.ctx)
        g = L.ggml_new_graph(c.ctx)
        for t in first + list(outs.values()):
            L.ggml_build_forward_expand(g, t)
        buf = L.ggml_backend_alloc_ctx_tensors(cl.ctx, backend)
        ga = L.ggml_gallocr_new(L.ggml_backend_get_default_buffer_type(backend))
        assert buf and ga and L.ggml_gallocr_alloc_graph(ga, g)
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return read(L, outs["out"]), L.ggml_backend_mi355x_last_launch_count(backend), L.ggml_gallocr_get_buffer_size(ga, 0)
        finally:
            L.ggml_gallocr_free(ga)
            L.ggml_backend_buffer_free(buf)


def rel_err(got, ref):
    ref = ref.astype(np.float64)
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def same_bits(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()


# ------------------------------------------------------------------ norm chain (try_fuse_norm, k_norm)

EPS = 1e-5


def norm_x(b, E, rows, strided=False):
    if strided:  # the first E of 2 E wide rows; the rest holds NaN
        full = np.full((rows, 2 * E), np.nan, np.float32)
        full[:, :E] = u(1, E * rows, 3.0, 0.5).reshape(rows, E)
        X = b.leaf("x", full, 2 * E, rows)
        return b.L.ggml_view_2d(b.c, X, E, rows, X.contents.nb[1], 0)
    return b.leaf("x", u(1, E * rows, 3.0, 0.5), E, rows)


def norm_of(b, x, rms):
    return (b.L.ggml_rms_norm if rms else b.L.ggml_norm)(b.c, x, EPS)


def vec_g(b, E, rows, kind="vec"):
    L, c = b.L, b.c
    if kind == "full":
        return b.leaf("g", u(2, E * rows, 1.0, 1.5), E, rows)
    if kind == "strided":  # a column of an [2, E] leaf: ne [E, 1], nb[0] = 8
        G2 = b.leaf("g", u(2, 2 * E, 1.0, 1.5), 2, E)
        return L.ggml_transpose(c, L.ggml_view_2d(c, G2, 1, E, 8, 0))
    return b.leaf("g", u(2, E, 1.0, 1.5), E)


def vec_b(b, E, rows, kind="vec"):
    if kind == "full":
        return b.leaf("b", u(3, E * rows, 2.0), E, rows)
    return b.leaf("b", u(3, E, 2.0), E)


def norm_chain(b, E, rows, rms, bias, strided=False, second=None, flag=False, g_kind="vec", b_kind="vec", swap=False):
    L, c = b.L, b.c
    n = norm_of(b, norm_x(b, E, rows, strided), rms)
    m = L.ggml_mul(c, n, vec_g(b, E, rows, g_kind))
    out = m
    if bias:
        bt = vec_b(b, E, rows, b_kind)
        out = L.ggml_add(c, bt, m) if swap else L.ggml_add(c, m, bt)
    outs = {"out": out}
    if flag:
        outs["norm"] = flag_output(n)
    if second:
        t = n if second == "norm" else m
        outs[second] = t
        outs[second + "_reader"] = L.ggml_scale(c, t, 0.5)
    return outs


GB = {"g": "out", "b": "out"}
for E in (96, 256):
    for rows in (1, 3):
        s = f"E{E}-r{rows}"
        add(f"norm/norm-mul-add/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True), True, absorbed=2, absorbable=GB)
        add(f"norm/rms-mul/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, True, False), True, absorbed=1, absorbable={"g": "out"})
        add(f"norm/rms-mul-add/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, True, True), True, absorbed=2, absorbable=GB)
        add(f"norm/strided-input/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True, strided=True), True, absorbed=2,
            absorbable=GB)
        add(f"norm/near/norm-second-reader/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True, second="norm"), False,
            absorbable=GB)
        add(f"norm/near/mul-second-reader/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, True, True, second="mul"), False,
            absorbable=GB)
        add(f"norm/near/norm-flagged-output/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True, flag=True), False,
            absorbable=GB)
        add(f"norm/near/g-full-shape/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, True, True, g_kind="full"), False, absorbable=GB)
        add(f"norm/near/g-strided/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True, g_kind="strided"), False, absorbable=GB)
        add(f"norm/near/bias-full-shape/{s}", lambda b, E=E, r=rows: norm_chain(b, E, r, False, True, b_kind="full"), False,
            absorbable=GB)
    add(f"norm/near/add-b-mul/E{E}-r1", lambda b, E=E: norm_chain(b, E, 1, False, True, swap=True), False, absorbable=GB)


def long_norm(b, rms, chain=False, inplace=False):
    L, c = b.L, b.c
    x = b.leaf("x", u(4, LONG_ROW * 2, 3.0, 0.5), LONG_ROW, 2)
    if inplace:
        return {"out": rms_norm_inplace(L, c, x, EPS)}
    n = norm_of(b, x, rms)
    if chain:
        n = L.ggml_add(c, L.ggml_mul(c, n, b.leaf("g", u(2, LONG_ROW, 1.0, 1.5), LONG_ROW)), b.leaf("b", u(3, LONG_ROW, 2.0), LONG_ROW))
    return {"out": n}


add("norm/long-row/norm", lambda b: long_norm(b, False), True)
add("norm/long-row/rms", lambda b: long_norm(b, True), True)
add("norm/long-row/norm-mul-add", lambda b: long_norm(b, False, chain=True), True, absorbed=2, absorbable=GB)
add("norm/long-row/rms-mul-add", lambda b: long_norm(b, True, chain=True), True, absorbed=2, absorbable=GB)
add("norm/long-row/rms-inplace", lambda b: long_norm(b, True, inplace=True), True)


# ------------------------------------------------------------------ norm chain as a GEMV's prologue

def norm_gemv(b, wtype, K, cols, rms, second=False):
    L, c = b.L, b.c
    n = norm_of(b, b.leaf("x", u(5, K * cols, 2.0, 0.25), K, cols), rms)
    h = L.ggml_add(c, L.ggml_mul(c, n, vec_g(b, K, cols)), vec_b(b, K, cols))
    outs = {"out": L.ggml_mul_mat(c, b.weight(wtype, K, N_OUT, 6), h)}
    if second:
        outs["h"] = h
        outs["out2"] = L.ggml_mul_mat(c, b.weight(wtype, K, N_OUT, 7), h)
    return outs


for rms in (False, True):
    nn = "rms" if rms else "norm"
    for K in (96, 1000):
        for cols in (1, 3, 8):
            add(f"prologue/f16/{nn}-K{K}-c{cols}", lambda b, K=K, cols=cols, rms=rms: norm_gemv(b, F16, K, cols, rms), True,
                absorbed=3, tol=TOL_F16, absorbable=GB)
    for wt in (Q4_K, Q8_0):
        for K in (256, 768):
            for cols in (1, 3):
                add(f"prologue/{TYPE_NAME[wt]}/{nn}-K{K}-c{cols}", lambda b, wt=wt, K=K, cols=cols, rms=rms: norm_gemv(b, wt, K, cols, rms),
                    True, absorbed=3, tol=TOL_Q, absorbable=GB)
        add(f"prologue/near/{TYPE_NAME[wt]}-K1024/{nn}", lambda b, wt=wt, rms=rms: norm_gemv(b, wt, 1024, 1, rms), False, tol=TOL_Q,
            absorbable=GB)
        add(f"prologue/near/{TYPE_NAME[wt]}-9-columns/{nn}", lambda b, wt=wt, rms=rms: norm_gemv(b, wt, 256, 9, rms), False, tol=TOL_Q,
            absorbable=GB)
        add(f"prologue/near/{TYPE_NAME[wt]}-second-mul-mat/{nn}", lambda b, wt=wt, rms=rms: norm_gemv(b, wt, 256, 3, rms, second=True),
            False, tol={"out": TOL_Q, "out2": TOL_Q}, absorbable=GB)
    add(f"prologue/near/f16-9-columns/{nn}", lambda b, rms=rms: norm_gemv(b, F16, 96, 9, rms), False, tol=TOL_F16, absorbable=GB)
    add(f"prologue/near/f16-second-mul-mat/{nn}", lambda b, rms=rms: norm_gemv(b, F16, 96, 3, rms, second=True), False,
        tol={"out": TOL_F16, "out2": TOL_F16}, absorbable=GB)


# ------------------------------------------------------------------ soft_max chain (try_fuse_softmax, k_soft_max)

def causal_mask(n_kv, N, n_past, dtype):
    m = np.zeros((N, n_kv), np.float32)
    for i in range(N):
        m[i, n_past + i + 1:] = -np.inf
    return m.astype(dtype)


def softmax_chain(b, n_kv, N, H, n_past, ne3=1, ext=False, second=None, mode="inf", mask=None, plain=False):
    L, c = b.L, b.c
    ne = (n_kv, N, H) if ne3 == 1 else (n_kv, N, H, ne3)
    x = b.leaf("x", u(8, n_kv * N * H * ne3, 4.0), *ne)
    if plain:
        return {"out": L.ggml_soft_max(c, x)}
    sc = L.ggml_scale(c, x, b.scale(1.0 / 8.0))
    dm = {"inf": L.ggml_diag_mask_inf, "zero": lambda c, a, n: diag_mask_zero(L, c, a, n),
          "inplace": lambda c, a, n: diag_mask_inf_inplace(L, c, a, n)}[mode](c, sc, n_past)
    if mask is not None:  # a second, additive mask that hides the first key as well
        m = causal_mask(n_kv, N, n_past, np.float16 if mask == F16 else np.float32)
        m[:, 0] = -3.0
        sm = L.ggml_soft_max_ext(c, dm, b.leaf("mask", m, n_kv, N, ttype=mask), 1.0, 0.0)
    elif ext:
        sm = L.ggml_soft_max_ext(c, dm, None, 0.5, 0.0)
    else:
        sm = L.ggml_soft_max(c, dm)
    outs = {"out": sm}
    if second:
        t = sc if second == "scale" else dm
        outs[second] = t
        outs[second + "_reader"] = L.ggml_scale(c, t, 0.5)
    return outs


SC = {"scale": "out"}
for n_kv, N, H, n_past in ((13, 1, 3, 12), (40, 8, 2, 32), (7, 7, 2, 0)):
    add(f"softmax/chain/kv{n_kv}-N{N}-H{H}", lambda b, a=(n_kv, N, H, n_past): softmax_chain(b, *a), True, absorbed=2, absorbable=SC)
add("softmax/chain/4d", lambda b: softmax_chain(b, 13, 3, 2, 10, ne3=2), True, absorbed=2, absorbable=SC)
add("softmax/chain/soft-max-ext-scale", lambda b: softmax_chain(b, 40, 8, 2, 32, ext=True), True, absorbed=2, absorbable=SC)
add("softmax/long-row/chain", lambda b: softmax_chain(b, LONG_ROW, 2, 1, LONG_ROW - 2), True, absorbed=2, absorbable=SC)
add("softmax/long-row/plain", lambda b: softmax_chain(b, LONG_ROW, 2, 1, 0, plain=True), True)
add("softmax/near/scale-second-reader", lambda b: softmax_chain(b, 40, 8, 2, 32, second="scale"), False, absorbable=SC)
add("softmax/near/mask-second-reader", lambda b: softmax_chain(b, 40, 8, 2, 32, second="mask"), False, absorbable=SC)
add("softmax/near/diag-mask-zero", lambda b: softmax_chain(b, 40, 8, 2, 32, mode="zero"), False, absorbable=SC)
add("softmax/near/ext-f32-mask", lambda b: softmax_chain(b, 40, 8, 2, 32, mask=F32), False, absorbable={"scale": "out", "mask": "out"})
add("softmax/near/ext-f16-mask", lambda b: softmax_chain(b, 40, 8, 2, 32, mask=F16), False, absorbable={"scale": "out", "mask": "out"})
add("softmax/near/diag-mask-inf-inplace", lambda b: softmax_chain(b, 40, 8, 2, 32, mode="inplace"), False, absorbable=SC)


# ------------------------------------------------------------------ GEMV epilogues (collect_epilogue)

def row_view(b, t, r0, r1, cols):
    return b.L.ggml_view_2d(b.c, t, r1 - r0, cols, t.contents.nb[1], 4 * r0)


def epilogue(b, wtype, K, cols, pat, N=N_OUT):
    L, c = b.L, b.c
    third = N // 3
    W = b.weight(wtype, K, N, 9)
    big = None
    if pat in ("cpy-over-x", "cpy-over-bias", "cpy-over-resid", "cpy-beside-x", "out-over-x"):
        # x, bias or resid at the start of one big leaf that the copy, or the output, lands in
        big = b.leaf("big", u(10, 8192, 2.0), 8192)
    if pat in ("cpy-over-x", "cpy-beside-x", "out-over-x"):
        x = L.ggml_view_2d(c, big, K, cols, 4 * K, 0)
    else:
        x = b.leaf("x", u(11, K * cols), K, cols)
    mm = L.ggml_mul_mat(c, W, x)
    bias = lambda: L.ggml_view_1d(c, big, N, 0) if pat == "cpy-over-bias" else b.leaf("bias", u(12, N, 2.0), N)
    resid = lambda: b.leaf("resid", u(13, N * cols, 2.0), N, cols)
    outs = {}
    if pat == "bias":
        out = L.ggml_add(c, mm, bias())
    elif pat == "bias-resid":
        out = L.ggml_add(c, L.ggml_add(c, mm, bias()), resid())
    elif pat == "bias-resid-strided":
        full = np.full((cols, 2 * N), np.nan, np.float32)
        full[:, :N] = u(13, N * cols, 2.0).reshape(cols, N)
        R = b.leaf("resid", full, 2 * N, cols)
        out = L.ggml_add(c, L.ggml_add(c, mm, bias()), L.ggml_view_2d(c, R, N, cols, R.contents.nb[1], 0))
    elif pat == "bias-gelu":
        out = L.ggml_gelu(c, L.ggml_add(c, mm, bias()))
    elif pat in ("bias-2cpy", "3cpy", "cpy-f16", "2cpy-overlapping-dst"):
        out = L.ggml_add(c, mm, bias())
        outs["out"] = out
        if pat == "2cpy-overlapping-dst":  # the second lands 16 floats into the first: the later one wins
            D = b.leaf("dst", np.zeros(third * cols + 16, np.float32), third * cols + 16)
            outs["cpy1"] = L.ggml_cpy(c, row_view(b, out, third, 2 * third, cols), L.ggml_view_1d(c, D, third * cols, 0))
            outs["cpy2"] = L.ggml_cpy(c, row_view(b, out, 2 * third, N, cols), L.ggml_view_1d(c, D, third * cols, 64))
            return outs
        ranges = {"bias-2cpy": [(third, 2 * third), (2 * third, N)], "3cpy": [(0, third), (third, 2 * third), (2 * third, N)],
                  "cpy-f16": [(third, 2 * third)]}[pat]
        for k, (r0, r1) in enumerate(ranges):
            dst = new(L, b.lc, F16 if pat == "cpy-f16" else F32, r1 - r0, cols)
            outs[f"cpy{k + 1}"] = L.ggml_cpy(c, row_view(b, out, r0, r1, cols), dst)
        return outs
    elif pat == "cpy-whole":
        out = L.ggml_add(c, mm, bias())
        return {"out": out, "cpy1": L.ggml_cpy(c, out, new(L, b.lc, F32, N, cols))}
    elif pat == "add-inplace":
        out = add_inplace(L, c, resid(), L.ggml_add(c, mm, bias()))
    elif pat == "out-over-x":
        # the residual, and with add_inplace the output, is a range of the big leaf that starts 16 floats into x:
        # the output aliases the residual element for element (legal) and overlaps x (every workgroup reads all
        # of x: the F16 GEMV first converts x into scratch, the quantized one refuses)
        out = add_inplace(L, c, L.ggml_view_2d(c, big, N, cols, 4 * N, 64), L.ggml_add(c, mm, bias()))
        return {"out": out, "big": big}
    elif pat == "cpy-over-out":
        # 8 rows of the result copied over later rows of its last column: the copy must run after the store
        out = L.ggml_add(c, mm, bias())
        return {"out": out, "cpy1": L.ggml_cpy(c, row_view(b, out, third, third + 8, cols), L.ggml_view_1d(c, out, 8 * cols, 4 * ((cols - 1) * N + third + 16)))}
    elif pat == "near-mm-second-reader":
        out = L.ggml_add(c, mm, bias())
        outs = {"mm": mm, "mm_reader": L.ggml_scale(c, mm, 0.5)}
    elif pat == "near-bias-sum-second-reader":
        s = L.ggml_add(c, mm, bias())
        out = L.ggml_gelu(c, s)
        outs = {"sum": s, "sum_reader": L.ggml_scale(c, s, 0.5)}
    elif pat == "near-bias-full-shape":
        out = L.ggml_add(c, mm, b.leaf("bias", u(12, N * cols, 2.0), N, cols))
    elif pat == "near-resid-broadcast":
        out = L.ggml_add(c, L.ggml_add(c, mm, bias()), b.leaf("resid", u(13, N, 2.0), N, 1))
    elif pat == "near-add-mm-mm":
        out = L.ggml_add(c, mm, mm)
    elif pat == "near-add-y-y":
        y = L.ggml_add(c, mm, bias())
        out = L.ggml_add(c, y, y)
    elif pat == "near-gelu-no-bias":
        out = L.ggml_gelu(c, mm)
    elif pat == "cpy-past-n":
        # rows [3N/4, 5N/4) of every column: past N, so into the next column (the last column's tail reads
        # past the tensor, into the guard leaf allocated behind it: those elements are not compared)
        out = L.ggml_add(c, mm, bias())
        b.leaf("guard", np.zeros(N, np.float32), N)
        r0, n = 3 * N // 4, N // 2
        outs = {"out": out, "cpy1": L.ggml_cpy(c, L.ggml_view_2d(c, out, n, cols, out.contents.nb[1], 4 * r0), new(L, b.lc, F32, n, cols))}
        ok = np.ones((cols, n), bool)
        ok[cols - 1, N - r0:] = False
        b.masks["cpy1"] = ok.reshape(-1)
        return outs
    elif pat in ("cpy-over-x", "cpy-beside-x", "cpy-over-bias", "cpy-over-resid"):
        # the copy's destination is a range of the big leaf: over the middle of x / the bias / the residual
        # (the copy must then run after the GEMV has read it), or right behind x
        n = third * cols
        if pat == "cpy-over-resid":
            out = L.ggml_add(c, L.ggml_add(c, mm, bias()), L.ggml_view_2d(c, big, N, cols, 4 * N, 0))
            at = 16
        else:
            out = L.ggml_add(c, mm, bias())
            at = {"cpy-over-x": 32, "cpy-beside-x": K * cols, "cpy-over-bias": 16}[pat]
        outs = {"out": out, "cpy1": L.ggml_cpy(c, row_view(b, out, third, 2 * third, cols), L.ggml_view_1d(c, big, n, 4 * at))}
        outs["big"] = big
        return outs
    else:
        raise KeyError(pat)
    outs = dict(out=out, **outs)
    return outs


EPI_POSITIVE = {"bias": 1, "bias-resid": 2, "bias-resid-strided": 2, "bias-gelu": 2, "bias-2cpy": 3, "cpy-whole": 2, "add-inplace": 2}
EPI_NEAR = ["near-mm-second-reader", "near-bias-sum-second-reader", "near-bias-full-shape", "near-resid-broadcast", "near-add-mm-mm",
            "near-add-y-y", "near-gelu-no-bias", "3cpy", "cpy-f16", "cpy-past-n", "2cpy-overlapping-dst", "cpy-over-x", "cpy-beside-x",
            "cpy-over-bias", "cpy-over-resid"]
EPI_WEIGHTS = [(F16, 96), (F16, 256)] + [(t, K) for t in (Q4_0, Q8_0, Q4_K, Q5_K, Q6_K) for K in (256, 512)]


def epi_tol(wtype, pat):
    base = TOL_F16 if wtype == F16 else TOL_Q
    gelu = TOL_GELU if "gelu" in pat or pat == "near-bias-sum-second-reader" else base
    return {"out": gelu, "cpy1": base, "cpy2": base, "cpy3": base, "mm": base, "mm_reader": base, "sum": base, "sum_reader": base,
            "big": base}


def epi_absorbable(pat):
    a = {}
    if pat not in ("near-add-mm-mm", "near-gelu-no-bias", "cpy-over-bias"):
        a["bias"] = "out"
    if "resid" in pat and pat != "cpy-over-resid" or pat == "add-inplace":
        a["resid"] = "out"
    return a


for wt, K in EPI_WEIGHTS:
    for cols in (1, 3):
        s = f"{TYPE_NAME[wt]}-K{K}-c{cols}"
        for pat, n_abs in EPI_POSITIVE.items():
            add(f"epilogue/{pat}/{s}", lambda b, a=(wt, K, cols, pat): epilogue(b, *a), True, absorbed=n_abs, tol=epi_tol(wt, pat),
                absorbable=epi_absorbable(pat))
        for pat in EPI_NEAR:
            if pat == "cpy-past-n" and cols == 1:
                continue  # one column has no next column to run into
            add(f"epilogue/near/{pat.replace('near-', '')}/{s}", lambda b, a=(wt, K, cols, pat): epilogue(b, *a), False,
                tol=epi_tol(wt, pat), absorbable=epi_absorbable(pat))
        # Refusals whose launch count is known, so a guard that lets them through fails the count, whatever the
        # race then does to the values. The output over x: the F16 GEMV still fuses, behind one launch that
        # converts x into scratch (3 nodes, 2 launches); overlaps(out, x) refuses the quantized one (3 launches).
        add(f"epilogue/aliased/out-over-x/{s}", lambda b, a=(wt, K, cols, "out-over-x"): epilogue(b, *a), True,
            absorbed=1 if wt == F16 else 0, tol=epi_tol(wt, "out-over-x"), absorbable={"bias": "out"})
        # a copy that lands in the result itself is not absorbed (overlaps(cp, out)): GEMV + bias, then the copy
        add(f"epilogue/aliased/cpy-over-out/{s}", lambda b, a=(wt, K, cols, "cpy-over-out"): epilogue(b, *a), True,
            absorbed=1, tol=epi_tol(wt, "cpy-over-out"), absorbable={"bias": "out"})
# the same with enough rows for many workgroups, where a missing guard also shows in the values
for wt in (F16, Q4_K):
    add(f"epilogue/aliased/out-over-x/{TYPE_NAME[wt]}-K256-c3-N2048", lambda b, wt=wt: epilogue(b, wt, 256, 3, "out-over-x", N=2048), True,
        absorbed=1 if wt == F16 else 0, tol=epi_tol(wt, "out-over-x"), absorbable={"bias": "out"})


# ------------------------------------------------------------------ copy batching (try_fuse_copies, k_cpy_multi)

def copies(b, pat):
    L, c = b.L, b.c
    a = b.leaf("a", u(14, 120), 40, 3)
    h = b.leaf("h", u(15, 85).astype(np.float16), 17, 5, ttype=F16)
    p = b.leaf("p", u(16, 192).astype(np.float16), 8, 6, 4, ttype=F16)
    t = b.leaf("t", u(17, 231), 33, 7)
    e = b.leaf("e", u(18, 120), 40, 3)

    def four():
        return {"f32-f16": L.ggml_cpy(c, a, new(L, b.lc, F16, 40, 3)), "f16-f32": L.ggml_cpy(c, h, new(L, b.lc, F32, 17, 5)),
                "permuted": L.ggml_cpy(c, L.ggml_permute(c, p, 1, 0, 2, 3), new(L, b.lc, F16, 6, 8, 4)),
                "out": L.ggml_cont(c, L.ggml_transpose(c, t))}
    if pat == "four":
        return four()
    if pat == "five":
        return dict(four(), fifth=L.ggml_cpy(c, e, new(L, b.lc, F32, 120)))
    c1 = L.ggml_cpy(c, a, new(L, b.lc, F32, 40, 3))
    if pat == "reads-first-dst":
        return {"cpy1": c1, "out": L.ggml_cpy(c, c1, new(L, b.lc, F16, 40, 3))}
    if pat == "writes-first-src":
        return {"cpy1": c1, "out": L.ggml_cpy(c, e, a)}
    if pat == "writes-first-dst":
        return {"out": L.ggml_cpy(c, L.ggml_view_1d(c, e, 60, 0), L.ggml_view_1d(c, c1, 60, 4 * 30)), "cpy1": c1}
    if pat == "node-between":
        return {"cpy1": c1, "scaled": L.ggml_scale(c, t, 0.5), "out": L.ggml_cpy(c, e, new(L, b.lc, F16, 40, 3))}
    raise KeyError(pat)


add("copies/four", lambda b: copies(b, "four"), True, absorbed=3)
add("copies/five", lambda b: copies(b, "five"), True, absorbed=3)  # 4 + 1
for pat in ("reads-first-dst", "writes-first-src", "writes-first-dst", "node-between"):
    add(f"copies/near/{pat}", lambda b, pat=pat: copies(b, pat), False)


# ------------------------------------------------------------------ embedding (try_fuse_embedding)

def embedding(b, wtype, E, pat="plain"):
    L, c = b.L, b.c
    V, P, N = 7, 16, 5
    ids, pos = np.array([6, 2, 6, 0, 3], np.int32), np.array([1, 0, 5, 15, 5], np.int32)
    wte = b.weight(wtype, E, V, 19) if pat != "2d-index" else new(L, b.lc, wtype, E, V, 2)
    if pat == "2d-index":
        b.feeds.append((wte, np.concatenate([weight_bytes(L, wtype, E, V, 19), weight_bytes(L, wtype, E, V, 20)])))
        wpe = b.leaf("wpe", u(21, E * P * 2, 2.0), E, P, 2)
        it, pt = b.leaf("ids", np.stack([ids, ids[::-1]]), N, 2, ttype=I32), b.leaf("pos", np.stack([pos, pos[::-1]]), N, 2, ttype=I32)
    else:
        Ep = E // 2 if pat == "different-widths" else E
        wpe = b.leaf("wpe", u(21, Ep * P, 2.0), Ep, P)
        it, pt = b.leaf("ids", ids, N, ttype=I32), b.leaf("pos", pos, N, ttype=I32)
    r1 = L.ggml_get_rows(c, wte, it)
    mid = L.ggml_scale(c, b.leaf("z", u(22, 8), 8), 0.5) if pat == "node-between" else None
    if mid:
        b.first += [r1, mid]
    r2 = L.ggml_get_rows(c, wpe, pt)
    outs = {"out": L.ggml_add(c, r2, r1) if pat == "swapped" else L.ggml_add(c, r1, r2)}
    if mid:
        outs["scaled"] = mid
    if pat == "second-reader":
        outs["rows"] = r1
        outs["rows_reader"] = L.ggml_scale(c, r1, 0.5)
    return outs


WPE = {"wpe": "out"}
for wt, E in ((F16, 96), (Q4_K, 512)):
    s = f"{TYPE_NAME[wt]}-E{E}"
    add(f"embedding/plain/{s}", lambda b, a=(wt, E): embedding(b, *a), True, absorbed=2, absorbable=WPE)  # index 6 repeats
    add(f"embedding/swapped/{s}", lambda b, a=(wt, E): embedding(b, *a, pat="swapped"), True, absorbed=2, absorbable=WPE)
    for pat in ("second-reader", "2d-index", "different-widths", "node-between"):
        add(f"embedding/near/{pat}/{s}", lambda b, a=(wt, E), pat=pat: embedding(b, *a, pat=pat), False, absorbable=WPE)


# ------------------------------------------------------------------ attention block (plan_attention, try_fuse_attn_proj)

D_HEAD, N_HEAD, N_CTX = 32, 4, 64


def attention(b, n_past, N, Hk=None, form="diag", near=None, proj=None, D=D_HEAD, H=N_HEAD):
    """The GPT-2 attention subgraph of test_gpt2_attention_block_exact at D = 32, H = 4, n_ctx = 64."""
    L, c = b.L, b.c
    Hk = Hk or H
    E, Ek, n_kv = D * H, D * Hk, n_past + N
    k16 = near == "k-cache-f16"
    cur = b.leaf("cur", u(23, (E + 2 * Ek) * N), E + 2 * Ek, N)
    mem_k = u(24, Ek * N_CTX)
    mk = b.leaf("mem_k", mem_k.astype(np.float16) if k16 else mem_k, Ek * N_CTX, ttype=F16 if k16 else F32)
    mv = b.leaf("mem_v", u(25, Ek * N_CTX), Ek * N_CTX)
    ksz = 2 if k16 else 4
    nb1 = cur.contents.nb[1]
    Qcur = L.ggml_view_2d(c, cur, E, N, nb1, 0)
    Kcur = L.ggml_view_2d(c, cur, Ek, N, nb1, 4 * E)
    Vcur = L.ggml_view_2d(c, cur, Ek, N, nb1, 4 * (E + Ek))
    ck = L.ggml_cpy(c, Kcur, L.ggml_view_1d(c, mk, N * Ek, ksz * Ek * n_past))
    cv = L.ggml_cpy(c, Vcur, L.ggml_view_1d(c, mv, N * Ek, 4 * Ek * n_past))
    qc = L.ggml_cont_3d(c, Qcur, D, H, N)
    Q = L.ggml_permute(c, qc, 0, 2, 1, 3)
    K = L.ggml_permute(c, L.ggml_reshape_3d(c, L.ggml_view_1d(c, mk, n_kv * Ek, 0), D, Hk, n_kv), 0, 2, 1, 3)
    KQ = L.ggml_mul_mat(c, K, Q)
    sc = L.ggml_scale(c, KQ, b.scale(1.0 / np.sqrt(D)))
    if form == "diag":
        dm = L.ggml_diag_mask_inf(c, sc, n_past)
    else:  # batched decode: an additive F32 mask, [n_kv, N] or (near-miss) one per head
        m = causal_mask(n_kv, N, n_past, np.float32)
        if near == "mask-per-head":
            dm = L.ggml_add(c, sc, b.leaf("mask", np.stack([m] * H), n_kv, N, H))
        else:
            dm = L.ggml_add(c, sc, b.leaf("mask", m, n_kv, N))
    sm = L.ggml_soft_max(c, dm)
    vsrc = L.ggml_permute(c, L.ggml_reshape_3d(c, L.ggml_view_1d(c, mv, n_kv * Ek, 0), D, Hk, n_kv), 1, 2, 0, 3)
    if near == "cont-v-reshaped":
        Vt = L.ggml_reshape_3d(c, L.ggml_cont(c, vsrc), n_kv, D, Hk)
    else:
        Vt = L.ggml_cont_3d(c, vsrc, n_kv, D, Hk)
    KQV = L.ggml_mul_mat(c, Vt, sm)
    att = L.ggml_cont_2d(c, L.ggml_permute(c, KQV, 0, 2, 1, 3), E, N)
    if near == "k-copy-after-kq":  # KQ reads the cache before this graph's K rows land in it
        b.first += [cv, KQ]
    outs = {"ck": ck, "cv": cv}
    if near == "soft-max-flagged-output":
        outs["sm"] = flag_output(sm)
    if near == "scaled-kq-second-reader":
        outs["sc"], outs["sc_reader"] = sc, L.ggml_scale(c, sc, 0.5)
    if near == "cont-q-second-reader":
        outs["qc"], outs["qc_reader"] = qc, L.ggml_scale(c, qc, 0.5)
    if not proj:
        outs["out"] = att
        return outs
    # + c_proj (F16) + bias + residual, then an LN -> F16 GEMV consumer or a plain one
    F = 2 * E
    O = L.ggml_add(c, L.ggml_add(c, L.ggml_mul_mat(c, b.weight(F16, E, E, 26), att), b.leaf("bias", u(27, E, 2.0), E)),
                   b.leaf("resid", u(28, E * N, 2.0), E, N))
    if proj == "ln_fc":
        h = L.ggml_add(c, L.ggml_mul(c, L.ggml_norm(c, O, EPS), vec_g(b, E, N)), vec_b(b, E, N))
        y = L.ggml_gelu(c, L.ggml_add(c, L.ggml_mul_mat(c, b.weight(F16, E, F, 29), h), b.leaf("bias_fc", u(30, F, 2.0), F)))
    else:
        y = L.ggml_add(c, O, O)
    outs["out"], outs["O"] = y, O
    return outs


# the block's ten nodes run as two launches: the K and V cache copies as one, and everything else at KQV
# (the cache copies, cont(Q) and its reader hold copied values: identical bits in either order)
ATT_TOL = {"out": TOL_ATTN, "sm": TOL_ATTN, "sc": TOL_ATTN, "sc_reader": TOL_ATTN}
ATT = dict(absorbed=8, tol=ATT_TOL, absorbable=SC)
for n_past, N in ((0, 1), (39, 1), (20, 5)):
    # (one key: its weight is 1 whatever the scale, so nothing is absorbable there)
    add(f"attention/block/past{n_past}-N{N}", lambda b, a=(n_past, N): attention(b, *a), True, **dict(ATT, absorbable=SC if n_past else {}))
add("attention/block/gqa-2-kv-heads", lambda b: attention(b, 20, 5, Hk=2), True, **ATT)
# the ADD of the mask is absorbed in place of the DIAG_MASK_INF
add("attention/block/additive-mask", lambda b: attention(b, 20, 5, form="add"), True, absorbed=8, tol=ATT_TOL,
    absorbable={"scale": "out", "mask": "out"})
# try_fuse_attn_proj takes head size 64 only (mi_attn_proj_supported: a.D == 64), so at D = 32 the projection
# stays a GEMV of its own with its bias and residual (3 nodes, 1 launch); ln_2 .. GELU (6 nodes) are 1 launch
add("attention/proj/ln_fc", lambda b: attention(b, 39, 1, proj="ln_fc"), True, absorbed=15, orders=(0,),
    tol={"ck": EXACT, "cv": EXACT, "O": TOL_ATTN, "out": TOL_GELU}, absorbable={"bias": "O", "resid": "O", "g": "out", "b": "out"})
add("attention/proj/plain", lambda b: attention(b, 39, 1, proj="plain"), True, absorbed=10, orders=(0,),
    tol={"ck": EXACT, "cv": EXACT, "O": TOL_ATTN, "out": TOL_ATTN}, absorbable={"bias": "O", "resid": "O"})
# at head size 64 (H = 2) it applies in tree order: the block, c_proj and its two ADDs are one k_attn_proj launch
# whose partial sums the LN -> GEMV consumer adds in its prologue (3 launches for 19 nodes); any other consumer
# has mi_sum_parts store them first (4 for 14). In the reference order the counts are those of D = 32.
add("attention/proj/d64-ln_fc", lambda b: attention(b, 39, 1, proj="ln_fc", D=64, H=2), True, absorbed={0: 16, 1: 15},
    tol={"ck": EXACT, "cv": EXACT, "O": TOL_ATTN, "out": TOL_GELU}, absorbable={"bias": "O", "resid": "O", "g": "out", "b": "out"})
add("attention/proj/d64-plain", lambda b: attention(b, 39, 1, proj="plain", D=64, H=2), True, absorbed=10,
    tol={"ck": EXACT, "cv": EXACT, "O": TOL_ATTN, "out": TOL_ATTN}, absorbable={"bias": "O", "resid": "O"})
for near in ("soft-max-flagged-output", "scaled-kq-second-reader", "cont-q-second-reader", "cont-v-reshaped", "k-cache-f16",
             "k-copy-after-kq"):
    add(f"attention/near/{near}", lambda b, near=near: attention(b, 20, 5, near=near), False, tol=ATT_TOL, absorbable=SC)
add("attention/near/mask-per-head", lambda b: attention(b, 20, 5, form="add", near="mask-per-head"), False, tol=ATT_TOL,
    absorbable={"scale": "out", "mask": "out"})


# ------------------------------------------------------------------ under the graph allocator

GALLOCR = ["norm/rms-mul-add/E256-r3", "softmax/chain/kv40-N8-H2", "epilogue/bias-resid/f16-K256-c3", "epilogue/bias-resid/q4_K-K512-c3",
           "attention/block/past20-N5", "embedding/plain/f16-E96"]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
