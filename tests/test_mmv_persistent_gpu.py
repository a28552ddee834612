"""The sliced grouped decode GEMV (k_mmv_stream with mi_mmv_group::slice_rows > 0: the resident count
of workgroups, each member's rows dealt to its workgroups in interleaved 16-row slices) against the
contiguous partition that a positive mmv_blocks selects: the same rows run the same arithmetic, so
every output is bit-equal; both are within test_mul_mat_gpu.py's TOL of the CPU restatement.

Shapes: the smallest at which the slicing can go wrong. A launch is sliced when its workgroups would
get more than one slice of rows each, so among N in {4, 20, 36, 1003, 1028} the small ones keep the
contiguous ranges (and must be unchanged) and 1003 / 1028 with 33 or 64 members are sliced: a last slice
of 11 rows (the waves get 3, 3, 3, 2 of them) or of 4, workgroups with one slice more than others.
"""
import numpy as np
import pytest

import pyoracle as orc
from ggml_mi355x import ggml as G
from ggml_mi355x import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3  # tests/test_mul_mat_gpu.py: max |dy| / max |y| against the reference CPU mul_mat
GUARD = 64  # floats behind every dst


@pytest.fixture(scope="module")
def rt():
    return G.runtime()


@pytest.fixture(scope="module")
def backend(rt):
    b = G.mi355x_backend(rt, 0)
    yield b
    rt.ggml_backend_free(b)


def rel_err(y, ref):
    return float(np.abs(y.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


_weights = {}


def weights(t, K, N):
    """One quantized N x K matrix per (type, K, N) and its rows as a 2-D byte array."""
    if (t, K, N) not in _weights:
        wq = orc.quantize(t, synth.uniform(7 + N, K * N), K)
        _weights[(t, K, N)] = wq.reshape(N, orc.row_size(t, K))
    return _weights[(t, K, N)]


def run_group(rt, backend, t, K, N, B, R, blocks_list):
    """R independent mul_mats (member r: the matrix with its rows rotated by r, its own X) in one
    graph, computed twice in a row for every entry of blocks_list (mmv_blocks; 0: the default
    launch). dst is filled with NaNs before each compute and a guard tensor lies behind each dst.
    Returns {blocks: [y of compute 1, y of compute 2]}, the CPU restatement's y and the route."""
    w2 = weights(t, K, N)
    wqs = [np.ascontiguousarray(np.roll(w2, r, axis=0)).ravel() for r in range(R)]
    xs = [synth.uniform(100 + r, K * B) for r in range(R)]
    ref = np.stack([orc.mul_mat(t, wqs[r], K, N, xs[r], B) for r in range(R)])
    nan = np.full(N * B, np.nan, np.float32)
    guard = np.arange(GUARD, dtype=np.float32) + 0.5
    out = {}
    ovh = rt.ggml_tensor_overhead() * (4 * R + 8) + rt.ggml_graph_overhead_custom(4 * R + 16, False)
    with G.Context(rt, ovh) as ctx:
        c = ctx.ctx
        wt = [rt.ggml_new_tensor_2d(c, t, K, N) for _ in range(R)]
        xt = [rt.ggml_new_tensor_2d(c, G.GGML_TYPE_F32, K, B) for _ in range(R)]
        yt, gt = [], []
        for r in range(R):
            yt.append(rt.ggml_mul_mat(c, wt[r], xt[r]))
            gt.append(rt.ggml_new_tensor_1d(c, G.GGML_TYPE_F32, GUARD))
        g = rt.ggml_new_graph_custom(c, 4 * R + 16, False)
        for y in yt:
            rt.ggml_build_forward_expand(g, y)
        buf = rt.ggml_backend_alloc_ctx_tensors(c, backend)
        assert buf
        try:
            for r in range(R):
                G.tensor_set(rt, wt[r], wqs[r])
                G.tensor_set(rt, xt[r], xs[r])
                G.tensor_set(rt, gt[r], guard)
            for blocks in blocks_list:
                assert rt.ggml_backend_mi355x_set_tuning(b"mmv_blocks", blocks)
                out[blocks] = []
                for _ in range(2):
                    for y in yt:
                        G.tensor_set(rt, y, nan)
                    assert rt.ggml_backend_graph_compute(backend, g) == G.GGML_STATUS_SUCCESS
                    assert rt.ggml_backend_mi355x_last_launch_count(backend) == 1
                    out[blocks].append(np.stack([G.tensor_get(rt, y) for y in yt]))
            route = rt.ggml_backend_mi355x_last_mul_mat_route(backend).decode()
            for r in range(R):
                assert np.array_equal(G.tensor_get(rt, gt[r]), guard), f"member {r}: written past dst"
        finally:
            rt.ggml_backend_mi355x_set_tuning(b"mmv_blocks", 0)
            rt.ggml_backend_buffer_free(buf)
    return out, ref, route


def check(out, ref, route, what):
    assert route.startswith("k_mmv_stream<") and ",ord0,pro0,mr1,ids0>" in route, route
    base = out[0][0]
    assert not np.isnan(base).any(), f"{what}: rows left unwritten"
    err = rel_err(base, ref)
    print(f"{what}: {route}, rel err {err:.2e}")
    assert err <= TOL, what
    for blocks, ys in out.items():
        for i, y in enumerate(ys):
            assert np.array_equal(y.view(np.uint32), base.view(np.uint32)), f"{what}: mmv_blocks={blocks}, compute {i + 1}"


CASES = [("q4_K", 256), ("q4_K", 512), ("q5_K", 256), ("q5_K", 512), ("q8_0", 256), ("q4_0", 256)]


@pytest.mark.parametrize("R", [1, 3, 33])
@pytest.mark.parametrize("tname,K", CASES)
def test_default_launch_bit_equal_to_contiguous_ranges(rt, backend, tname, K, R):
    t = orc.TYPES_BY_NAME[tname]
    for N in (4, 20, 36, 1003, 1028):
        for B in (1, 2, 8):
            # the contiguous partition at about the resident count and at twice it (the two grids of
            # the launcher before the slices)
            out, ref, route = run_group(rt, backend, t, K, N, B, R, [0, 1024, 2048])
            check(out, ref, route, f"{tname} K={K} N={N} B={B} x{R}")


@pytest.mark.parametrize("tname", ["q4_K", "q5_K", "q8_0", "q4_0"])
def test_many_slices_per_workgroup(rt, backend, tname):
    """N = 8192 at K = 256: far more slices (512 a member) than workgroups of a member, 64 members
    (the most of one launch: the fewest workgroups each); the contiguous side on few, long ranges."""
    t = orc.TYPES_BY_NAME[tname]
    out, ref, route = run_group(rt, backend, t, 256, 8192, 1, 64, [0, 128])
    check(out, ref, route, f"{tname} K=256 N=8192 x64")
