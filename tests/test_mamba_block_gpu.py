"""One Mamba layer end to end on MI355X against the reference CPU: the graph llama.cpp's build_mamba makes
at this ggml vintage, through the same ggml calls on the same bytes on both sides.

  state views * state_mask -> rms_norm * g -> ssm_in mul_mat -> x / z views -> ssm_conv -> cpy of columns 1 ..
  of the conv states into the cache -> + bias -> silu -> ssm_x mul_mat -> dt / B / C views -> ssm_dt mul_mat
  + bias -> ssm_scan -> cpy of the states into the cache -> y + x * D -> * silu(z) -> ssm_out mul_mat

(the layer without its residual add, which would bury the layer's own output under the input)

d_model 256, d_inner 512, d_state 16, d_conv 4, dt_rank 16. A prompt (5 or 40 tokens, state_mask 0: the cache's
old contents are cleared) is followed by two decode steps on the cache each side carried over itself, with
one sequence and with two sequences in one batch.

Bars, NMSE against the reference CPU at every step, on the layer output and on both caches:
  * F32 weights: <= 1e-7, the reference harness's default max_nmse_err (the scan's expf / log1pf are not
    the CPU's bits).
  * Q4_K ssm_in / ssm_x / ssm_out (ssm_dt stays F32: K = 16): <= 5e-4, the harness's bar for quantized
    mul_mats: a last-ulp difference from expf becomes a whole quant step where the next mul_mat
    re-quantizes its input, as in the opt-out path of tests/test_llama_block_gpu.py.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
from ssm_cases import nmse, run_graph, uniform

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]

F32, I32, Q4_K = G.GGML_TYPE_F32, G.GGML_TYPE_I32, G.GGML_TYPE_Q4_K
D_MODEL, D_INNER, D_STATE, D_CONV, DT_RANK = 256, 512, 16, 4, 16
BAR = {F32: 1e-7, Q4_K: 5e-4}


@pytest.fixture(scope="module")
def libs():
    rt = G.runtime()
    be = G.mi355x_backend(rt)
    ref = G.Lib([REF_LIB], isolated=True)
    cpu = ref.ggml_backend_cpu_init()
    ref.ggml_backend_cpu_set_n_threads(cpu, min(16, os.cpu_count() or 1))
    yield rt, be, ref, cpu
    ref.ggml_backend_free(cpu)
    rt.ggml_backend_free(be)


def _weights(wtype):
    rt = G.runtime()
    w = {}
    for i, (name, k, n, scale) in enumerate((("ssm_in", D_MODEL, 2 * D_INNER, 0.08), ("ssm_x", D_INNER, DT_RANK + 2 * D_STATE, 0.05),
                                             ("ssm_out", D_INNER, D_MODEL, 0.05))):
        f = (uniform(600 + i, n, k) * np.float32(scale)).astype(np.float32)
        if wtype == F32:
            w[name] = (F32, f, k, n)
        else:
            out = np.empty(G.row_size(wtype, k) * n, np.uint8)
            rt.ggml_quantize_chunk(wtype, f.ctypes.data, out.ctypes.data, 0, n, k, None)
            w[name] = (wtype, out, k, n)
    w["ssm_dt"] = (F32, (uniform(610, D_INNER, DT_RANK) * np.float32(0.5)).astype(np.float32), DT_RANK, D_INNER)
    w["norm"] = (1.0 + 0.1 * uniform(611, D_MODEL)).astype(np.float32)
    w["conv1d"] = (uniform(612, D_INNER, D_CONV) * np.float32(0.5)).astype(np.float32)
    w["conv1d_b"] = (uniform(613, D_INNER) * np.float32(0.1)).astype(np.float32)
    w["dt_b"] = (np.float32(2.0) * uniform(614, D_INNER)).astype(np.float32)
    w["A"] = (-(np.arange(D_STATE, dtype=np.float32) + np.float32(1.0))[None, :] *
              (np.float32(0.5) + np.abs(uniform(615, D_INNER, D_STATE)))).astype(np.float32)
    w["D"] = (1.0 + 0.1 * uniform(616, D_INNER)).astype(np.float32)
    return w


def _build(L, c, W, n_kv, x, sq, mask, conv_cache, ssm_cache):
    """x [T, D_MODEL], sq [T, n_kv] i32, mask [n_kv] f32, the caches as each side left them."""
    feeds = []

    def new(t, arr, *ne):
        tt = {1: L.ggml_new_tensor_1d, 2: L.ggml_new_tensor_2d}[len(ne)](c, t, *ne)
        feeds.append((tt, arr))
        return tt

    T = x.shape[0]
    inp = new(F32, x, D_MODEL, T)
    state_seq = new(I32, sq, n_kv, T)
    state_mask = new(F32, mask, 1, n_kv)
    k_l = new(F32, conv_cache, (D_CONV - 1) * D_INNER * n_kv)
    v_l = new(F32, ssm_cache, D_STATE * D_INNER * n_kv)
    wt = {k: new(v[0], v[1], v[2], v[3]) for k, v in W.items() if isinstance(v, tuple)}
    norm, conv1d, conv1d_b = new(F32, W["norm"], D_MODEL), new(F32, W["conv1d"], D_CONV, D_INNER), new(F32, W["conv1d_b"], D_INNER)
    dt_b, A, D = new(F32, W["dt_b"], D_INNER), new(F32, W["A"], D_STATE, D_INNER), new(F32, W["D"], D_INNER)

    conv_states = L.ggml_reshape_2d(c, k_l, (D_CONV - 1) * D_INNER, n_kv)
    ssm_states = L.ggml_reshape_2d(c, v_l, D_STATE * D_INNER, n_kv)
    # clear the states of sequences that start in this batch
    conv_states = L.ggml_mul(c, L.ggml_view_2d(c, conv_states, (D_CONV - 1) * D_INNER, n_kv, conv_states.contents.nb[1], 0), state_mask)
    ssm_states = L.ggml_mul(c, L.ggml_view_2d(c, ssm_states, D_STATE * D_INNER, n_kv, ssm_states.contents.nb[1], 0), state_mask)
    conv_states = L.ggml_reshape_3d(c, conv_states, D_CONV - 1, D_INNER, n_kv)
    ssm_states = L.ggml_reshape_3d(c, ssm_states, D_STATE, D_INNER, n_kv)

    cur = L.ggml_mul(c, L.ggml_rms_norm(c, inp, 1e-5), norm)
    xz = L.ggml_mul_mat(c, wt["ssm_in"], cur)
    row = xz.contents.nb[1]
    xv = L.ggml_view_2d(c, xz, D_INNER, T, row, 0)
    z = L.ggml_view_2d(c, xz, D_INNER, T, row, 4 * D_INNER)

    x_conv = L.ggml_ssm_conv(c, conv_states, xv, conv1d, state_seq)
    conv_cpy = L.ggml_cpy(c, L.ggml_view_2d(c, x_conv, D_CONV - 1, D_INNER * n_kv, D_CONV * 4, (1 + D_INNER * T) * 4),
                          L.ggml_view_1d(c, k_l, (D_CONV - 1) * D_INNER * n_kv, 0))
    xv = L.ggml_view_2d(c, x_conv, D_INNER, T, D_INNER * 4, 0)
    xv = L.ggml_silu(c, L.ggml_add(c, xv, conv1d_b))

    x_db = L.ggml_mul_mat(c, wt["ssm_x"], xv)
    row = x_db.contents.nb[1]
    dt = L.ggml_view_2d(c, x_db, DT_RANK, T, row, 0)
    B = L.ggml_view_2d(c, x_db, D_STATE, T, row, 4 * DT_RANK)
    C = L.ggml_view_2d(c, x_db, D_STATE, T, row, 4 * (DT_RANK + D_STATE))
    dt = L.ggml_add(c, L.ggml_mul_mat(c, wt["ssm_dt"], dt), dt_b)
    y_states = L.ggml_ssm_scan(c, ssm_states, xv, dt, A, B, C, state_seq)
    ssm_cpy = L.ggml_cpy(c, L.ggml_view_1d(c, y_states, D_STATE * D_INNER * n_kv, D_INNER * T * 4),
                         L.ggml_view_1d(c, v_l, D_STATE * D_INNER * n_kv, 0))
    y = L.ggml_view_2d(c, y_states, D_INNER, T, D_INNER * 4, 0)
    y = L.ggml_add(c, y, L.ggml_mul(c, xv, D))
    y = L.ggml_mul(c, y, L.ggml_silu(c, z))
    out = L.ggml_mul_mat(c, wt["ssm_out"], y)
    # the cache writes go into the graph ahead of the output, as llama.cpp expands them
    return feeds, [("conv_cache", conv_cpy), ("ssm_cache", ssm_cpy), ("out", out)]


def _batch(n_kv, T, decode):
    """sq [T, n_kv]: one id per token. Two sequences: a decode step holds one token of each; a prompt
    gives sequence 0 the first 60% of the tokens, then alternates."""
    sq = np.full((T, n_kv), -1, np.int32)
    if n_kv == 1:
        sq[:, 0] = 0
    elif decode:
        sq[:, 0] = np.arange(T) % n_kv
    else:
        head = (3 * T) // 5
        sq[:head, 0] = 0
        sq[head:, 0] = (np.arange(T - head) + 1) % n_kv
    return sq


@pytest.mark.parametrize("n_kv", [1, 2], ids=["one_sequence", "two_sequences"])
@pytest.mark.parametrize("prompt", [5, 40])
@pytest.mark.parametrize("wtype", [F32, Q4_K], ids=["f32", "q4_K"])
def test_mamba_layer(libs, wtype, prompt, n_kv):
    rt, be, ref, cpu = libs
    W = _weights(wtype)
    # the cache's old contents, cleared by the prompt's state_mask
    caches = {side: [uniform(620, (D_CONV - 1) * D_INNER * n_kv), uniform(621, D_STATE * D_INNER * n_kv)] for side in ("dev", "cpu")}
    steps = [(prompt, False), (n_kv, True), (n_kv, True)]
    for i, (T, decode) in enumerate(steps):
        x = (uniform(630 + i, T, D_MODEL) * np.float32(2.0)).astype(np.float32)
        sq = _batch(n_kv, T, decode)
        mask = np.full(n_kv, 1.0 if decode else 0.0, np.float32)
        res = {}
        for side, L, b in (("dev", rt, be), ("cpu", ref, cpu)):
            cc, sc = caches[side]
            res[side] = run_graph(L, b, lambda L_, c: _build(L_, c, W, n_kv, x, sq, mask, cc, sc), n_tensors=128)
            caches[side] = [res[side]["conv_cache"], res[side]["ssm_cache"]]
        for name in ("out", "conv_cache", "ssm_cache"):
            a, want = res["dev"][name], res["cpu"][name]
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(a)), (i, name)
            e = nmse(a, want)
            print(f"mamba layer {'f32' if wtype == F32 else 'q4_K'} n_kv={n_kv} step {i} (T={T}) {name}: NMSE {e:.3e}")
            assert e <= BAR[wtype], (i, name, e)
