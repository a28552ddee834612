"""GGML_OP_MUL_MAT_ID (the expert-routed mul_mat of mixture-of-experts graphs) on MI355X against the
reference CPU: the same graph through both libraries on the same bytes.

c[:, e, t] = as[:, :, ids[e, t]] . b[:, e % ne11, t] with every pair through the weight type's
vec_dot on from_float-quantized activations -- the arithmetic of MUL_MAT per column. So in the
reference order (mmv_order 1) the result is the reference CPU's bits, and in tree order it is held to
the project's standing bar max|d| / max|y| <= 1e-5. The ids stay on the device: the kernels look the
expert up, on every path (pair by pair, grouped by expert, streaming decode kernel).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
from ggml_mi355x import synth

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]

F32, F16, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_F16, G.GGML_TYPE_I32
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 12, 13, 14
NAMES = {0: "f32", 1: "f16", 2: "q4_0", 3: "q4_1", 6: "q5_0", 7: "q5_1", 8: "q8_0", 12: "q4_K", 13: "q5_K", 14: "q6_K"}
K_TYPES = (Q4_K, Q5_K, Q6_K)
ALL_TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K, F16, F32)
N = 100  # a row tail for every kernel (4, 32 and 64 rows per workgroup)


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


_weights = {}


def experts(t, K, n, n_as, seed=11):
    """n_as expert matrices [K, n] of type t as raw bytes (quantized by the runtime's ggml_quantize_chunk)."""
    key = (t, K, n, n_as, seed)
    if key not in _weights:
        f = (synth.uniform(seed + t, K * n * n_as) * np.float32(0.08)).astype(np.float32)
        if t == F32:
            w = f.view(np.uint8)
        elif t == F16:
            w = f.astype(np.float16).view(np.uint8)
        else:
            w = np.empty(G.row_size(t, K) * n * n_as, np.uint8)
            G.runtime().ggml_quantize_chunk(t, f.ctypes.data, w.ctypes.data, 0, n * n_as, K, None)
        _weights[key] = w
    return _weights[key]


def random_ids(n_as, T, seed):
    """[T, n_as] rows, each a permutation of the experts (as the reference harness fills them)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n_as) for _ in range(T)]).astype(np.int32)


def build_mmid(L, c, t, w, K, n, n_as, n_ids, ne11, T, x, ids_full):
    """ids_full: [T, width] int32; the op reads the first n_ids entries of every row (a strided view
    when width > n_ids)."""
    width = ids_full.shape[1]
    a = L.ggml_new_tensor_3d(c, t, K, n, n_as)
    b = L.ggml_new_tensor_3d(c, F32, K, ne11, T)
    full = L.ggml_new_tensor_2d(c, I32, width, T)
    ids = full if width == n_ids else L.ggml_view_2d(c, full, n_ids, T, full.contents.nb[1], 0)
    y = L.ggml_mul_mat_id(c, a, b, ids)
    return [(a, w), (b, x), (full, ids_full)], y


def both(libs, t, K, n, n_as, n_ids, ne11, T, ids_full, seed=5):
    rt, be, ref, cpu = libs
    w = experts(t, K, n, n_as)
    x = (synth.uniform(seed, K * ne11 * T) * np.float32(2.0)).astype(np.float32)
    a = G.graph_once(rt, be, lambda c: build_mmid(rt, c, t, w, K, n, n_as, n_ids, ne11, T, x, ids_full)[0:2])
    b = G.graph_once(ref, cpu, lambda c: build_mmid(ref, c, t, w, K, n, n_as, n_ids, ne11, T, x, ids_full)[0:2])
    return a, b


def check(a, b, order, what):
    if order == 1:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: not the reference's bits, identical {np.mean(a == b):.4f}"
    else:
        rel = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        assert rel <= 1e-5, f"{what}: max|d| / max|y| = {rel:.2e}"


class tuning:
    """set_tuning for the duration of a with block (the process-wide knobs are restored)."""

    def __init__(self, rt, **kv):
        self.rt, self.kv = rt, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.rt.ggml_backend_mi355x_set_tuning(k.encode(), v[0]), k

    def __exit__(self, *a):
        for k, v in self.kv.items():
            self.rt.ggml_backend_mi355x_set_tuning(k.encode(), v[1])


# (K, n_as, n_ids, b broadcast, n_tokens): every value of every axis at least once per type;
# K = 288 (ragged: 9 blocks of 32) for the 32-block types and F16 / F32
SHAPES = [(256, 4, 1, False, 1), (512, 8, 2, True, 1), (256, 8, 4, False, 3), (512, 4, 2, False, 8), (256, 8, 2, True, 9),
          (512, 4, 4, True, 33), (256, 8, 4, False, 33)]
RAGGED = [(288, 4, 2, True, 1), (288, 8, 2, False, 33)]


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: NAMES[t])
def test_types_and_orders(libs, t, order):
    rt = libs[0]
    with tuning(rt, mmv_order=(order, -1)):
        for i, (K, n_as, n_ids, bc, T) in enumerate(SHAPES + ([] if t in K_TYPES else RAGGED)):
            ne11 = 1 if bc else n_ids
            a, b = both(libs, t, K, N, n_as, n_ids, ne11, T, random_ids(n_as, T, 40 + i))
            assert a.shape == (N * n_ids * T,)
            check(a, b, order, f"{NAMES[t]} K={K} n_as={n_as} n_ids={n_ids} ne11={ne11} T={T}")


def _patterns(n_as, T):
    r = random_ids(n_as, T, 3)
    unused = np.where(r >= n_as - 1, (r + 1) % (n_as - 1), r)  # the last expert: selected by no token
    one = np.full((T, n_as), 2, np.int32)                        # every pair on expert 2
    twice = r.copy()
    twice[:, 1] = twice[:, 0]                                    # one expert twice in a row of ids
    return {"strided": r, "unused": unused, "one_expert": one, "twice": twice}


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("pattern", ["strided", "unused", "one_expert", "twice"])
@pytest.mark.parametrize("t", [Q4_K, Q5_0, F16], ids=lambda t: NAMES[t])
def test_id_patterns(libs, t, pattern, order):
    """33 tokens, 2 of 8 experts, ids a [2, 33] view of an [8, 33] tensor (row stride n_as)."""
    rt = libs[0]
    n_as, T = 8, 33
    ids = _patterns(n_as, T)[pattern]
    if pattern == "unused":
        assert (n_as - 1) not in ids[:, :2]
    with tuning(rt, mmv_order=(order, -1)):
        a, b = both(libs, t, 256, N, n_as, 2, 2, T, ids)
        check(a, b, order, f"{NAMES[t]} {pattern}")


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("t", [Q4_K, Q6_K, Q5_1], ids=lambda t: NAMES[t])
def test_grouped_equals_pairwise(libs, t, order):
    """Grouping the pairs by expert (mmid_group 1: where the backend's crossover applies it; 8 / 4:
    at any token count, up to 8 / 4 gathered columns per workgroup) keeps each column's own
    accumulators: bit-identical to the pairwise path (mmid_group 0) in both orders."""
    rt, be = libs[0], libs[1]
    for T, n_as, n_ids, ne11 in ((3, 4, 2, 1), (33, 8, 2, 2), (33, 4, 4, 4)):
        ids = random_ids(n_as, T, 9)
        w = experts(t, 256, N, n_as)
        x = (synth.uniform(6, 256 * ne11 * T) * np.float32(2.0)).astype(np.float32)
        outs = {}
        for grp in (0, 1, 8, 4):
            with tuning(rt, mmv_order=(order, -1), mmid_group=(grp, 1), mmid_stream=(1, 8)):
                outs[grp] = G.graph_once(rt, be, lambda c: build_mmid(rt, c, t, w, 256, N, n_as, n_ids, ne11, T, x, ids)[0:2])
        for grp in (1, 8, 4):
            assert np.array_equal(outs[grp].view(np.uint32), outs[0].view(np.uint32)), (NAMES[t], T, n_as, n_ids, grp)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import test_mul_mat_id_gpu as M
from ggml_mi355x import ggml as G
rt = G.runtime()
be = G.mi355x_backend(rt)
assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", 1)
outs = []
for t, K, n_as, n_ids, ne11 in M.DECODE_CASES:
    w = M.experts(t, K, M.N, n_as)
    x = (M.synth.uniform(8, K * ne11) * np.float32(2.0)).astype(np.float32)
    ids = M.random_ids(n_as, 1, 21)
    outs.append(G.graph_once(rt, be, lambda c: M.build_mmid(rt, c, t, w, K, M.N, n_as, n_ids, ne11, 1, x, ids)[0:2]))
np.save(sys.argv[2], np.concatenate(outs))
"""

DECODE_CASES = [(t, 512, 8, 2, ne11) for t in (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K) for ne11 in (1, 2)]


def test_streaming_equals_generic(libs, tmp_path):
    """One token of a streaming shape (K % 256 == 0, aligned experts) runs the streaming decode
    kernel with the device-resolved weight base; a child process with GGML_MI355X_NO_FUSED_MMV=1 runs
    the generic GEMV. Reference order: the same bits, and the reference CPU's."""
    rt, be, ref, cpu = libs
    out = str(tmp_path / "generic.npy")
    env = dict(os.environ, GGML_MI355X_NO_FUSED_MMV="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(os.path.abspath(__file__)), out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    generic = np.load(out)
    outs, refs = [], []
    with tuning(rt, mmv_order=(1, -1)):
        for t, K, n_as, n_ids, ne11 in DECODE_CASES:
            w = experts(t, K, N, n_as)
            x = (synth.uniform(8, K * ne11) * np.float32(2.0)).astype(np.float32)
            ids = random_ids(n_as, 1, 21)
            outs.append(G.graph_once(rt, be, lambda c: build_mmid(rt, c, t, w, K, N, n_as, n_ids, ne11, 1, x, ids)[0:2]))
            refs.append(G.graph_once(ref, cpu, lambda c: build_mmid(ref, c, t, w, K, N, n_as, n_ids, ne11, 1, x, ids)[0:2]))
    stream = np.concatenate(outs)
    assert np.array_equal(stream.view(np.uint32), generic.view(np.uint32))
    assert np.array_equal(stream.view(np.uint32), np.concatenate(refs).view(np.uint32))


# ---- a mixture-of-experts feed-forward block ----
E, FF, N_EXPERT, N_USED = 256, 512, 4, 2


def _moe_weights():
    return {"gate": experts(Q4_K, E, FF, N_EXPERT, 31), "up": experts(Q4_K, E, FF, N_EXPERT, 32), "down": experts(Q4_K, FF, E, N_EXPERT, 33),
            "g": (1.0 + 0.1 * synth.uniform(34, E)).astype(np.float32)}


def build_moe(L, c, W, T, x, ids, rw):
    """rms_norm -> mul(g) -> mul_mat_id(gate), mul_mat_id(up) -> silu(gate) * up -> mul_mat_id(down)
    -> * routing weights -> sum over the used experts (views + add). Returns (feeds, out, tensors)."""
    xt = L.ggml_new_tensor_2d(c, F32, E, T)
    gt = L.ggml_new_tensor_1d(c, F32, E)
    wg = L.ggml_new_tensor_3d(c, Q4_K, E, FF, N_EXPERT)
    wu = L.ggml_new_tensor_3d(c, Q4_K, E, FF, N_EXPERT)
    wd = L.ggml_new_tensor_3d(c, Q4_K, FF, E, N_EXPERT)
    idt = L.ggml_new_tensor_2d(c, I32, N_USED, T)
    rwt = L.ggml_new_tensor_3d(c, F32, 1, N_USED, T)
    h = L.ggml_mul(c, L.ggml_rms_norm(c, xt, 1e-5), gt)
    h3 = L.ggml_reshape_3d(c, h, E, 1, T)
    gate = L.ggml_mul_mat_id(c, wg, h3, idt)        # [FF, N_USED, T], b broadcast
    up = L.ggml_mul_mat_id(c, wu, h3, idt)
    par = L.ggml_mul(c, L.ggml_silu(c, gate), up)
    down = L.ggml_mul_mat_id(c, wd, par, idt)       # b [FF, N_USED, T]: not broadcast
    down = L.ggml_mul(c, down, rwt)                 # routing weights, broadcast over the rows
    nb = down.contents.nb
    out = None
    for e in range(N_USED):
        v = L.ggml_view_2d(c, down, E, T, nb[2], e * nb[1])
        out = v if out is None else L.ggml_add(c, out, v)
    feeds = [(xt, x), (gt, W["g"]), (wg, W["gate"]), (wu, W["up"]), (wd, W["down"]), (idt, ids), (rwt, rw)]
    return feeds, out, idt


def _moe_inputs(T, seed):
    x = (synth.uniform(seed, E * T) * np.float32(2.0)).astype(np.float32)
    ids = random_ids(N_EXPERT, T, seed)[:, :N_USED].copy()
    rw = (0.5 + 0.4 * synth.uniform(seed + 1, N_USED * T)).astype(np.float32)
    return x, ids, rw


@pytest.mark.parametrize("T", [1, 5, 12])
def test_moe_block_default_settings_bit_identical(libs, T):
    """No tuning set: graph_decode_order sees the quantized MUL_MAT_IDs that consume computed values
    and runs the graph in the reference order -- the block output is the reference CPU's bits."""
    rt, be, ref, cpu = libs
    W = _moe_weights()
    x, ids, rw = _moe_inputs(T, 50 + T)
    a = G.graph_once(rt, be, lambda c: build_moe(rt, c, W, T, x, ids, rw)[0:2], n_tensors=64)
    print(f"MoE block T={T}: {rt.ggml_backend_mi355x_last_launch_count(be)} kernel launches")
    b = G.graph_once(ref, cpu, lambda c: build_moe(ref, c, W, T, x, ids, rw)[0:2], n_tensors=64)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"identical {np.mean(a == b):.4f}"


def _stats(rt, be):
    arr = (ctypes.c_int64 * 6)()
    assert rt.ggml_backend_mi355x_graph_stats_ex(be, arr, 6) == 6
    return list(arr)


def test_ids_are_read_on_the_device(libs):
    """A decode MoE graph under graph capture: computed, captured, then only `ids` overwritten with
    ggml_backend_tensor_set and the same graph computed again. The capture is replayed (or updated in
    place), not taken anew, and both results are the reference's for their own ids."""
    rt, _, ref, cpu = libs
    be = G.mi355x_backend(rt)  # a backend of its own: fresh capture cache and counters
    W = _moe_weights()
    x, ids_a, rw = _moe_inputs(1, 70)
    ids_b = ((ids_a + 1) % N_EXPERT).astype(np.int32)
    want = [G.graph_once(ref, cpu, lambda c: build_moe(ref, c, W, 1, x, i, rw)[0:2], n_tensors=64) for i in (ids_a, ids_b)]
    ctx = G.Context(rt, rt.ggml_tensor_overhead() * 64 + rt.ggml_graph_overhead(), no_alloc=True)
    try:
        feeds, out, idt = build_moe(rt, ctx.ctx, W, 1, x, ids_a, rw)
        g = rt.ggml_new_graph(ctx.ctx)
        rt.ggml_build_forward_expand(g, out)
        buf = rt.ggml_backend_alloc_ctx_tensors(ctx.ctx, be)
        assert buf
        for t, arr in feeds:
            G.tensor_set(rt, t, arr)
        s0 = _stats(rt, be)
        for _ in range(2):  # the first graph of a topology is launched directly, the second captured
            assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
        got_a = G.tensor_get(rt, out)
        s1 = _stats(rt, be)
        assert s1[5] - s0[5] == 1, (s0, s1)
        G.tensor_set(rt, idt, ids_b)
        assert rt.ggml_backend_graph_compute(be, g) == G.GGML_STATUS_SUCCESS
        got_b = G.tensor_get(rt, out)
        s2 = _stats(rt, be)
        assert s2[5] == s1[5] and s2[3] == s1[3], (s1, s2)                    # no new capture, no direct launch
        assert (s2[4] - s1[4]) + (s2[2] - s1[2]) == 1, (s1, s2)              # a replay or an in-place update
        assert np.array_equal(got_a.view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got_b.view(np.uint32), want[1].view(np.uint32))
        assert not np.array_equal(want[0], want[1])
        rt.ggml_backend_buffer_free(buf)
    finally:
        ctx.free()
        rt.ggml_backend_free(be)
