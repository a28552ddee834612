"""ggml_mul_mat_id in the runtime core (src/ggml.c:4852-4897): the node the runtime's builder makes
equals the reference's in op, type, ne, nb and source order, for broadcast and non-broadcast b and
for ids given as a strided view (the reference harness's [n_used, n] view of an [n_mats, n] tensor).
"""
import ctypes
import os

import pytest

from conftest import REPO
from ggml_mi355x import ggml as G

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")

F32, I32, Q4_K, Q8_0, F16 = G.GGML_TYPE_F32, G.GGML_TYPE_I32, G.GGML_TYPE_Q4_K, G.GGML_TYPE_Q8_0, G.GGML_TYPE_F16
GGML_OP_MUL_MAT_ID = 24

# (type_a, K, N, n_as, n_ids, ne11, n_tokens, ids as a view of [n_as, n_tokens])
CASES = [
    (Q4_K, 256, 100, 8, 2, 2, 1, True),    # decode, not broadcast, the harness's strided ids
    (Q4_K, 256, 100, 8, 2, 1, 1, True),    # b broadcast over the used experts
    (Q8_0, 288, 100, 4, 4, 4, 33, False),  # every expert used: ids contiguous
    (F16, 512, 64, 4, 4, 2, 9, False),     # partial broadcast (n_ids % ne11 == 0)
    (F32, 32, 32, 8, 1, 1, 3, True),
]


def _describe(t):
    c = t.contents
    return dict(type=c.type, op=c.op, ne=tuple(c.ne), nb=tuple(c.nb), view_offs=c.view_offs, has_view_src=bool(c.view_src))


def _node(L, case):
    ta, K, N, n_as, n_ids, ne11, T, view = case
    with G.Context(L, L.ggml_tensor_overhead() * 8, no_alloc=True) as c:
        a = L.ggml_new_tensor_3d(c.ctx, ta, K, N, n_as)
        b = L.ggml_new_tensor_3d(c.ctx, F32, K, ne11, T)
        if view:
            full = L.ggml_new_tensor_2d(c.ctx, I32, n_as, T)
            ids = L.ggml_view_2d(c.ctx, full, n_ids, T, full.contents.nb[1], 0)
        else:
            ids = L.ggml_new_tensor_2d(c.ctx, I32, n_ids, T)
        r = L.ggml_mul_mat_id(c.ctx, a, b, ids)
        rc = r.contents
        addr = lambda t: ctypes.cast(t, ctypes.c_void_p).value
        src = [rc.src[i] for i in range(10)]
        d = _describe(r)
        d["src_is"] = (src[0] == addr(a), src[1] == addr(b), src[2] == addr(ids), all(s is None for s in src[3:]))
        d["src"] = [_describe(t) for t in (a, b, ids)]
        d["grad"] = bool(rc.grad)
        return d


def test_binding_exists():
    rt = G.runtime()
    assert rt.has("ggml_mul_mat_id")
    assert rt.ggml_op_name(GGML_OP_MUL_MAT_ID) == b"MUL_MAT_ID"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_node_shape(case):
    ta, K, N, n_as, n_ids, ne11, T, view = case
    d = _node(G.runtime(), case)
    assert d["op"] == GGML_OP_MUL_MAT_ID and d["type"] == F32
    assert d["ne"] == (N, n_ids, T, 1)
    assert d["nb"] == (4, 4 * N, 4 * N * n_ids, 4 * N * n_ids * T)
    assert d["src_is"] == (True, True, True, True)
    assert d["src"][2]["nb"][1] == 4 * (n_as if view else n_ids)


@needs_ref
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_node_equals_reference(case):
    ref = G.Lib([REF_LIB], isolated=True)
    assert _node(G.runtime(), case) == _node(ref, case)
