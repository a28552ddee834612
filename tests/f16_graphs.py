"""The ggml graphs of tests/f16_cases.py, built the same way for the reference CPU library
(tests/test_f16_cases.py) and for the MI355X backend (tests/test_f16_cases_gpu.py): the F16 mul_mat, its src1
in several layouts, the norm chain in front of it and the bias / residual / GELU nodes and row copies
behind it, node by node as GPT-2's graph has them."""
import numpy as np

from ggml_mi355x import ggml as G

import f16_cases as fc

F32, F16 = G.GGML_TYPE_F32, G.GGML_TYPE_F16
PAD_VALUE = np.float32(3.0e4)  # what lies between the columns of a strided src1 (never read by a correct kernel)


def build(L, c, m, src1="f32"):
    """-> feeds, [y, copy destinations ...], extra nodes to expand before y.
    src1: "f32" contiguous columns; "f16" the same values as an F16 tensor (the case's activations must be
    f16 values); "strided": a view of a [K + 4, B] tensor (columns 16 bytes aligned, K % 4 == 0);
    "unaligned": a view of a [K + 1, B] tensor (columns 4 bytes aligned only)."""
    K, N, B = m["K"], m["N"], m["B"]
    w = L.ggml_new_tensor_2d(c, F16, K, N)
    feeds = [(w, m["w16"])]
    if src1 == "f16":
        assert m.get("norm") is None and np.array_equal(m["xh"].astype(np.float32), m["x32"]), "src1 f16 needs f16-valued activations"
        x = L.ggml_new_tensor_2d(c, F16, K, B)
        feeds.append((x, m["xh"]))
    elif src1 == "f32":
        x = L.ggml_new_tensor_2d(c, F32, K, B)
        feeds.append((x, m["x32"]))
    else:
        pad = 4 if src1 == "strided" else 1
        parent = L.ggml_new_tensor_2d(c, F32, K + pad, B)
        buf = np.full((B, K + pad), PAD_VALUE, np.float32)
        buf[:, :K] = m["x32"]
        feeds.append((parent, buf))
        x = L.ggml_view_2d(c, parent, K, B, parent.contents.nb[1], 0)
    h = x
    norm = m.get("norm")
    if norm:
        h = (L.ggml_norm if norm["mode"] == fc.NORM else L.ggml_rms_norm)(c, x, float(norm["eps"]))
        if norm["g"] is not None:
            g = L.ggml_new_tensor_1d(c, F32, K)
            feeds.append((g, norm["g"].astype(np.float32)))
            h = L.ggml_mul(c, h, g)
        if norm["b"] is not None:
            b = L.ggml_new_tensor_1d(c, F32, K)
            feeds.append((b, norm["b"].astype(np.float32)))
            h = L.ggml_add(c, h, b)
    y = L.ggml_mul_mat(c, w, h)
    if m["bias"] is not None:
        bi = L.ggml_new_tensor_1d(c, F32, N)
        feeds.append((bi, m["bias"]))
        y = L.ggml_add(c, y, bi)
    if m["resid"] is not None:  # after the bias, as the separate nodes do
        rs = L.ggml_new_tensor_2d(c, F32, N, B)
        feeds.append((rs, m["resid"]))
        y = L.ggml_add(c, y, rs)
    if m.get("gelu"):
        y = L.ggml_gelu(c, y)
    outs, extra = [y], []
    for r0, r1 in m.get("copies") or []:
        dst = L.ggml_new_tensor_2d(c, F32, r1 - r0, B)
        extra.append(L.ggml_cpy(c, L.ggml_view_2d(c, y, r1 - r0, B, y.contents.nb[1], 4 * r0), dst))
        outs.append(dst)
    return feeds, outs, extra


def run(L, backend, m, src1="f32", n_tensors=48, repeat=1, after=None):
    """Builds and computes the case's graph `repeat` times on `backend`; returns the outputs of every
    compute as [[y [B, N], copies ...], ...] (one list when repeat == 1). after(L, backend): called after
    each compute, its values are returned as a second list."""
    overhead = L.ggml_tensor_overhead() * n_tensors + L.ggml_graph_overhead()
    with G.Context(L, overhead, no_alloc=True) as ctx:
        feeds, outs, extra = build(L, ctx.ctx, m, src1)
        g = L.ggml_new_graph(ctx.ctx)
        L.ggml_build_forward_expand(g, outs[0])
        for e in extra:
            L.ggml_build_forward_expand(g, e)
        buf = L.ggml_backend_alloc_ctx_tensors(ctx.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            res, notes = [], []
            for _ in range(repeat):
                assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                if after:
                    notes.append(after(L, backend))
                res.append([G.tensor_get(L, o).reshape(m["B"], -1) for o in outs])
        finally:
            L.ggml_backend_buffer_free(buf)
    if after:
        return (res[0], notes[0]) if repeat == 1 else (res, notes)
    return res[0] if repeat == 1 else res


def expected(m):
    """[y bits [B, N], the copies' bits ...] of a class-E case."""
    y = fc.expected_bits(m).reshape(m["B"], m["N"])
    return [y] + [y[:, r0:r1] for r0, r1 in m.get("copies") or []]


def build_parts(L, c, p):
    """The attention block of f16_cases.parts_case, node by node as GPT-2's graph builds it (one token, n_past
    cached keys); consumer None: add(O, O) instead of LN -> c_fc. -> feeds, [y, O], the K / V cache copies."""
    E, H, D, n_past, n_kv = p["E"], p["H"], p["D"], p["n_past"], p["n_kv"]
    cur = L.ggml_new_tensor_2d(c, F32, 3 * E, 1)
    mk, mv = L.ggml_new_tensor_1d(c, F32, E * n_kv), L.ggml_new_tensor_1d(c, F32, E * n_kv)
    Wp, Bp, R = L.ggml_new_tensor_2d(c, F16, E, E), L.ggml_new_tensor_1d(c, F32, E), L.ggml_new_tensor_2d(c, F32, E, 1)
    feeds = [(cur, p["cur"]), (mk, p["mem_k"]), (mv, p["mem_v"]), (Wp, p["wp"]), (Bp, p["bp"]), (R, p["resid"])]
    nb1 = cur.contents.nb[1]
    Qcur = L.ggml_view_2d(c, cur, E, 1, nb1, 0)
    Kcur = L.ggml_view_2d(c, cur, E, 1, nb1, 4 * E)
    Vcur = L.ggml_view_2d(c, cur, E, 1, nb1, 8 * E)
    ck = L.ggml_cpy(c, Kcur, L.ggml_view_1d(c, mk, E, 4 * E * n_past))
    cv = L.ggml_cpy(c, Vcur, L.ggml_view_1d(c, mv, E, 4 * E * n_past))
    Q = L.ggml_permute(c, L.ggml_cont_3d(c, Qcur, D, H, 1), 0, 2, 1, 3)
    K = L.ggml_permute(c, L.ggml_reshape_3d(c, L.ggml_view_1d(c, mk, n_kv * E, 0), D, H, n_kv), 0, 2, 1, 3)
    sm = L.ggml_soft_max(c, L.ggml_diag_mask_inf(c, L.ggml_scale(c, L.ggml_mul_mat(c, K, Q), 1.0 / np.sqrt(D)), n_past))
    Vt = L.ggml_cont_3d(c, L.ggml_permute(c, L.ggml_reshape_3d(c, L.ggml_view_1d(c, mv, n_kv * E, 0), D, H, n_kv), 1, 2, 0, 3), n_kv, D, H)
    att = L.ggml_cont_2d(c, L.ggml_permute(c, L.ggml_mul_mat(c, Vt, sm), 0, 2, 1, 3), E, 1)
    O = L.ggml_add(c, L.ggml_add(c, L.ggml_mul_mat(c, Wp, att), Bp), R)
    m = p["consumer"]
    if m is None:
        return feeds, [L.ggml_add(c, O, O), O], [ck, cv]
    norm = m["norm"]
    h = (L.ggml_norm if norm["mode"] == fc.NORM else L.ggml_rms_norm)(c, O, float(norm["eps"]))
    g = L.ggml_new_tensor_1d(c, F32, E)
    feeds.append((g, norm["g"].astype(np.float32)))
    h = L.ggml_mul(c, h, g)
    if norm["b"] is not None:
        b = L.ggml_new_tensor_1d(c, F32, E)
        feeds.append((b, norm["b"].astype(np.float32)))
        h = L.ggml_add(c, h, b)
    Wf = L.ggml_new_tensor_2d(c, F16, E, p["F"])
    feeds.append((Wf, m["w16"]))
    y = L.ggml_mul_mat(c, Wf, h)
    if m["bias"] is not None:
        bi = L.ggml_new_tensor_1d(c, F32, p["F"])
        feeds.append((bi, m["bias"]))
        y = L.ggml_add(c, y, bi)
    if m["resid"] is not None:
        rs = L.ggml_new_tensor_2d(c, F32, p["F"], 1)
        feeds.append((rs, m["resid"]))
        y = L.ggml_add(c, y, rs)
    if m.get("gelu"):
        y = L.ggml_gelu(c, y)
    return feeds, [y, O], [ck, cv]


def run_parts(L, backend, p, after=None):
    """-> [y, O] (and after(L, backend)'s value)."""
    overhead = L.ggml_tensor_overhead() * 96 + L.ggml_graph_overhead()
    with G.Context(L, overhead, no_alloc=True) as ctx:
        feeds, outs, extra = build_parts(L, ctx.ctx, p)
        g = L.ggml_new_graph(ctx.ctx)
        for e in extra:
            L.ggml_build_forward_expand(g, e)
        for o in outs:
            L.ggml_build_forward_expand(g, o)
        buf = L.ggml_backend_alloc_ctx_tensors(ctx.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            note = after(L, backend) if after else None
            res = [G.tensor_get(L, o) for o in outs]
        finally:
            L.ggml_backend_buffer_free(buf)
    return (res, note) if after else res


def expected_parts(p):
    """[y bits, O bits]."""
    o = np.ascontiguousarray(p["target"]).view(np.uint32)
    m = p["consumer"]
    y = fc.expected_bits(m).ravel() if m is not None else (p["target"] * np.float32(2)).view(np.uint32)
    return [y, o]


def aliased_case(cid="E-epi-resid", K=136, N=70, B=3):
    """mul_mat + bias + residual whose residual (and, added in place, output) is a range of the leaf that holds
    src1, 16 floats in: the output aliases the residual element for element and overlaps src1. The residual's
    values are the src1 values that lie there; the case is evaluated again with them."""
    base = fc.materialize(cid, K, N, B)
    assert 16 + N * B <= K * B
    d = dict(w=base["w"], x=base["x"], bias=base["bias"].astype(np.float64),
             resid=base["x32"].ravel()[16:16 + N * B].reshape(B, N).astype(np.float64))
    d.update(fc.evaluate(d, K))
    d.update(id=cid + "-aliased", cls="E", K=K, N=N, B=B)
    return d


def run_aliased(L, backend, m, after=None):
    import fusion_cases as FC
    K, N, B = m["K"], m["N"], m["B"]
    overhead = L.ggml_tensor_overhead() * 32 + L.ggml_graph_overhead()
    with G.Context(L, overhead, no_alloc=True) as ctx:
        c = ctx.ctx
        w = L.ggml_new_tensor_2d(c, F16, K, N)
        big = L.ggml_new_tensor_1d(c, F32, K * B)
        bi = L.ggml_new_tensor_1d(c, F32, N)
        x = L.ggml_view_2d(c, big, K, B, 4 * K, 0)
        r = L.ggml_view_2d(c, big, N, B, 4 * N, 64)
        y = FC.add_inplace(L, c, r, L.ggml_add(c, L.ggml_mul_mat(c, w, x), bi))
        g = L.ggml_new_graph(c)
        L.ggml_build_forward_expand(g, y)
        buf = L.ggml_backend_alloc_ctx_tensors(c, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in ((w, m["w16"]), (big, m["x32"]), (bi, m["bias"])):
                G.tensor_set(L, t, arr)
            assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            note = after(L, backend) if after else None
            out = G.tensor_get(L, big)[16:16 + N * B].reshape(B, N)
        finally:
            L.ggml_backend_buffer_free(buf)
    return (out, note) if after else out
