"""GGML_OP_SSM_CONV / GGML_OP_SSM_SCAN cases shared by tests/test_ssm.py (CPU) and tests/test_ssm_gpu.py:
seeded inputs, the graph of one node built through any library exporting the ggml API, and numpy
evaluations of the reference forwards (src/ggml.c:16311-16418, :16437-16543).

Layouts. numpy arrays are C-ordered with ggml's ne reversed: s [n_kv, d_inner, d_conv - 1 | d_state],
x / dt [n_t, d_inner], c [d_inner, d_conv], A [d_inner, d_state], B / C [n_t, d_state], sq [n_t, n_kv] i32.
dst is 1-D: the outputs [n_t, d_inner], then the new states [n_kv, d_inner, d_conv | d_state].

Sequences (both ops): with n_kv > 1 every state is first copied from src to dst; token t then updates the
state of sequence sq[t, 0] and copies it to sq[t, 1], sq[t, 2], .. up to the first id outside [0, n_kv).
The conv's dst states are one column wider than its src states: the copy fills columns 1 .., and column 0
of a sequence no token writes stays whatever the buffer held (NaN in `ConvCase.model`).
"""
import numpy as np

from ggml_mi355x import ggml as G
from ggml_mi355x import synth

F32, F16, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32
BAR_CPU = 1e-7  # the reference harness's default max_nmse_err (tests/test-backend-ops.cpp:288)


def uniform(seed, *shape):
    return synth.uniform(seed, int(np.prod(shape))).reshape(shape).astype(np.float32)


def nmse(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(np.sum((a - b) ** 2) / np.sum(b ** 2))


def run_graph(L, backend, build, n_tensors=96):
    """build(L, ctx) -> (feeds, outs): outs is a list of (name, tensor), expanded into the graph in order.
    Returns name -> f32 array of the tensor's bytes."""
    with G.Context(L, L.ggml_tensor_overhead() * n_tensors + L.ggml_graph_overhead(), no_alloc=True) as c:
        feeds, outs = build(L, c.ctx)
        g = L.ggml_new_graph(c.ctx)
        for _, t in outs:
            L.ggml_build_forward_expand(g, t)
        buf = L.ggml_backend_alloc_ctx_tensors(c.ctx, backend)
        assert buf, "buffer allocation failed"
        try:
            for t, arr in feeds:
                G.tensor_set(L, t, arr)
            assert L.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
            return {name: G.tensor_get(L, t, np.float32) for name, t in outs}
        finally:
            L.ggml_backend_buffer_free(buf)


def single_sequence(n_t):
    return np.zeros((n_t, 1), np.int32)


def walk_sequences(sq, n_kv, update, copy):
    """The token loop both forwards share; returns the set of sequences some token wrote."""
    written = set()
    for t in range(sq.shape[0]):
        s0 = int(sq[t, 0])
        assert 0 <= s0 < n_kv, "the reference aborts here; no test feeds such a token"
        update(t, s0)
        written.add(s0)
        for i3 in range(1, n_kv):
            to = int(sq[t, i3])
            if not 0 <= to < n_kv:
                break
            copy(s0, to)
            written.add(to)
    return written


class ConvCase:
    """One SSM_CONV node. strided: x is the first half of the rows of a [2 * d_inner, n_t] tensor (the
    x / z projection of a Mamba layer); the other half holds NaN."""

    def __init__(self, d_conv, d_inner, n_t, n_kv=1, sq=None, strided=False, seed=1):
        self.d_conv, self.d_inner, self.n_t, self.n_kv, self.strided = d_conv, d_inner, n_t, n_kv, strided
        self.s = uniform(seed, n_kv, d_inner, d_conv - 1)
        self.x = uniform(seed + 1, n_t, d_inner)
        self.c = uniform(seed + 2, d_inner, d_conv)
        self.sq = single_sequence(n_t) if sq is None else np.asarray(sq, np.int32).reshape(n_t, n_kv)
        self.what = f"conv d_conv={d_conv} d_inner={d_inner} n_t={n_t} n_kv={n_kv} strided={strided}"

    def node(self, L, c, feeds):
        s = L.ggml_new_tensor_3d(c, F32, self.d_conv - 1, self.d_inner, self.n_kv)
        if self.strided:
            xz = L.ggml_new_tensor_2d(c, F32, 2 * self.d_inner, self.n_t)
            full = np.full((self.n_t, 2 * self.d_inner), np.nan, np.float32)
            full[:, :self.d_inner] = self.x
            feeds.append((xz, full))
            x = L.ggml_view_2d(c, xz, self.d_inner, self.n_t, xz.contents.nb[1], 0)
        else:
            x = L.ggml_new_tensor_2d(c, F32, self.d_inner, self.n_t)
            feeds.append((x, self.x))
        w = L.ggml_new_tensor_2d(c, F32, self.d_conv, self.d_inner)
        sq = L.ggml_new_tensor_2d(c, I32, self.n_kv, self.n_t)
        feeds += [(s, self.s), (w, self.c), (sq, self.sq)]
        self.sq_tensor = sq
        return L.ggml_ssm_conv(c, s, x, w, sq)

    def build(self, L, c):
        feeds = []
        return feeds, [("out", self.node(L, c, feeds))]

    def split(self, out):
        n = self.n_t * self.d_inner
        return out[:n].reshape(self.n_t, self.d_inner), out[n:].reshape(self.n_kv, self.d_inner, self.d_conv)

    def model(self, unfused=None):
        """The reference forward in f32. The dot runs from 0.0f in column order; its first `unfused` terms
        are a rounded product added with a second rounding, the rest fused multiply-adds. The default,
        4 * (d_conv // 4), is what the reference's gcc -O3 -mfma build computes: it vectorizes the loop
        four columns at a time without fusing and contracts only the scalar remainder.
        (A fused step is evaluated in f64 and rounded to f32: the product of two f32 is exact in f64.)
        Returns y, states (NaN where the reference writes nothing) and the written sequences."""
        if unfused is None:
            unfused = 4 * (self.d_conv // 4)
        st = np.full((self.n_kv, self.d_inner, self.d_conv), np.nan, np.float32)
        st[:, :, 1:] = self.s
        y = np.empty((self.n_t, self.d_inner), np.float32)

        def update(t, s0):
            st[s0, :, :-1] = st[s0, :, 1:].copy()
            st[s0, :, -1] = self.x[t]
            acc = np.zeros(self.d_inner, np.float32)
            for i in range(self.d_conv):
                if i >= unfused:
                    acc = (st[s0, :, i].astype(np.float64) * self.c[:, i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
                else:
                    acc = acc + st[s0, :, i] * self.c[:, i]
            y[t] = acc

        def copy(s0, to):
            st[to] = st[s0]

        written = walk_sequences(self.sq, self.n_kv, update, copy)
        return y, st, written


class ScanCase:
    """One SSM_SCAN node. strided: B and C are views of a [dt_rank + 2 * d_state, n_t] tensor (the x_db
    projection of a Mamba layer) whose first dt_rank rows hold NaN."""
    DT_RANK = 5

    def __init__(self, d_state, d_inner, n_t, n_kv=1, sq=None, strided=False, seed=1):
        self.d_state, self.d_inner, self.n_t, self.n_kv, self.strided = d_state, d_inner, n_t, n_kv, strided
        self.s = uniform(seed, n_kv, d_inner, d_state)
        self.x = uniform(seed + 1, n_t, d_inner)
        # dt in [-4, 6], a few entries above 20 (the branch that skips the softplus)
        self.dt = (np.float32(1.0) + np.float32(5.0) * uniform(seed + 2, n_t, d_inner)).astype(np.float32)
        flat = self.dt.reshape(-1)
        flat[3::37] = np.float32(20.5)
        flat[11::101] = np.float32(33.0)
        # A[i0, i1] = -(i0 + 1) (0.5 + u), u = |uniform| in [0, 1]: negative, as in Mamba
        u = np.abs(uniform(seed + 3, d_inner, d_state))
        self.A = (-(np.arange(d_state, dtype=np.float32) + np.float32(1.0))[None, :] * (np.float32(0.5) + u)).astype(np.float32)
        self.B = uniform(seed + 4, n_t, d_state)
        self.C = uniform(seed + 5, n_t, d_state)
        self.sq = single_sequence(n_t) if sq is None else np.asarray(sq, np.int32).reshape(n_t, n_kv)
        self.what = f"scan d_state={d_state} d_inner={d_inner} n_t={n_t} n_kv={n_kv} strided={strided}"

    def node(self, L, c, feeds):
        s = L.ggml_new_tensor_3d(c, F32, self.d_state, self.d_inner, self.n_kv)
        x = L.ggml_new_tensor_2d(c, F32, self.d_inner, self.n_t)
        dt = L.ggml_new_tensor_2d(c, F32, self.d_inner, self.n_t)
        A = L.ggml_new_tensor_2d(c, F32, self.d_state, self.d_inner)
        if self.strided:
            r, n = self.DT_RANK, self.d_state
            x_db = L.ggml_new_tensor_2d(c, F32, r + 2 * n, self.n_t)
            full = np.full((self.n_t, r + 2 * n), np.nan, np.float32)
            full[:, r:r + n] = self.B
            full[:, r + n:] = self.C
            feeds.append((x_db, full))
            B = L.ggml_view_2d(c, x_db, n, self.n_t, x_db.contents.nb[1], 4 * r)
            C = L.ggml_view_2d(c, x_db, n, self.n_t, x_db.contents.nb[1], 4 * (r + n))
        else:
            B = L.ggml_new_tensor_2d(c, F32, self.d_state, self.n_t)
            C = L.ggml_new_tensor_2d(c, F32, self.d_state, self.n_t)
            feeds += [(B, self.B), (C, self.C)]
        sq = L.ggml_new_tensor_2d(c, I32, self.n_kv, self.n_t)
        feeds += [(s, self.s), (x, self.x), (dt, self.dt), (A, self.A), (sq, self.sq)]
        self.sq_tensor = sq
        return L.ggml_ssm_scan(c, s, x, dt, A, B, C, sq)

    def build(self, L, c):
        feeds = []
        return feeds, [("out", self.node(L, c, feeds))]

    def split(self, out):
        n = self.n_t * self.d_inner
        return out[:n].reshape(self.n_t, self.d_inner), out[n:].reshape(self.n_kv, self.d_inner, self.d_state)

    def exact(self):
        """The forward in f64 over the same f32 inputs: y, states."""
        st = self.s.astype(np.float64)
        y = np.empty((self.n_t, self.d_inner), np.float64)
        A, dt64 = self.A.astype(np.float64), self.dt.astype(np.float64)
        dtsp = np.where(self.dt <= np.float32(20.0), np.log1p(np.exp(dt64)), dt64)

        def update(t, s0):
            dA = np.exp(dtsp[t][:, None] * A)
            dBx = self.B[t].astype(np.float64)[None, :] * (self.x[t].astype(np.float64) * dtsp[t])[:, None]
            st[s0] = st[s0] * dA + dBx
            y[t] = st[s0] @ self.C[t].astype(np.float64)

        def copy(s0, to):
            st[to] = st[s0]

        walk_sequences(self.sq, self.n_kv, update, copy)
        return y, st


def check_scan(dev, cpu, exact, what):
    """The two bars of an SSM_SCAN result (y or the states), NMSE = sum((a - b)^2) / sum(b^2):
      1. NMSE(device, reference CPU) <= 1e-7
      2. NMSE(device, f64) <= 4 * NMSE(reference CPU, f64): a factor 2 in RMS, for expf / log1pf of the same
         1-ulp class as the CPU's libm and a tree-ordered 16-term sum (skipped where the CPU's is 0)."""
    assert np.all(np.isfinite(dev)), what
    e_cpu, e_dev, e_ref = nmse(dev, cpu), nmse(dev, exact), nmse(cpu, exact)
    print(f"{what}: NMSE device/cpu {e_cpu:.3e}, device/f64 {e_dev:.3e}, cpu/f64 {e_ref:.3e}")
    assert e_cpu <= BAR_CPU, (what, e_cpu)
    if e_ref > 0.0:
        assert e_dev <= 4.0 * e_ref, (what, e_dev, e_ref)
