"""The router builders of the runtime core -- ggml_argsort, ggml_top_k, ggml_sum_rows, ggml_div, ggml_sub
(src/ggml.c:6425, :6444, :4321, :4186, :4098): the node each makes equals the reference library's in
type, op, ne, nb, op_params, view offset, view source and sources.
"""
import ctypes
import os

import pytest

from conftest import REPO
from ggml_mi355x import ggml as G

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")

F32, I32 = G.GGML_TYPE_F32, G.GGML_TYPE_I32
ASC, DESC = 0, 1
BUILDERS = ("ggml_argsort", "ggml_top_k", "ggml_sum_rows", "ggml_div", "ggml_sub", "ggml_view_4d", "ggml_reshape_2d")


def _addr(t):
    return ctypes.cast(t, ctypes.c_void_p).value


def _describe(t, known):
    """Every compared field of a node; pointers as the name of the tensor they point at."""
    c = t.contents
    who = lambda p: known.get(p, "?") if p else None
    return dict(type=c.type, op=c.op, ne=tuple(c.ne), nb=tuple(c.nb), op_params=tuple(c.op_params), view_offs=c.view_offs,
                view_src=who(c.view_src), src=[who(c.src[i]) for i in range(10)], grad=bool(c.grad))


def _argsort(order):
    def build(L, c):
        a = L.ggml_new_tensor_4d(c, F32, 60, 3, 2, 1)
        r = L.ggml_argsort(c, a, order)
        return {"a": a, "r": r}
    return build


def _top_k(L, c):
    probs = L.ggml_new_tensor_2d(c, F32, 8, 5)
    r = L.ggml_top_k(c, probs, 2)
    # the argsort under the view: reached through the view's source
    s = ctypes.cast(r.contents.src[0], G.T)
    return {"probs": probs, "argsort": s, "r": r}


def _sum_rows(L, c):
    a = L.ggml_new_tensor_4d(c, F32, 7, 3, 2, 2)
    return {"a": a, "r": L.ggml_sum_rows(c, a)}


def _binary(name, same_shape):
    def build(L, c):
        a = L.ggml_new_tensor_2d(c, F32, 2, 5)
        b = L.ggml_new_tensor_2d(c, F32, 2 if same_shape else 1, 5)
        return {"a": a, "b": b, "r": getattr(L, name)(c, a, b)}
    return build


CASES = {
    "argsort_asc": _argsort(ASC),
    "argsort_desc": _argsort(DESC),
    "top_k": _top_k,
    "sum_rows": _sum_rows,
    "div_broadcast": _binary("ggml_div", False),   # [1, 5] against [2, 5]
    "div_same_shape": _binary("ggml_div", True),
    "sub": _binary("ggml_sub", True),              # (ggml_sub asserts equal shapes in the reference)
}


def _nodes(L, build):
    with G.Context(L, L.ggml_tensor_overhead() * 8, no_alloc=True) as c:
        ts = build(L, c.ctx)
        known = {_addr(t): name for name, t in ts.items()}
        return {name: _describe(t, known) for name, t in ts.items()}


def test_bindings_exist():
    rt = G.runtime()
    for name in BUILDERS:
        assert rt.has(name), name
    assert rt.ggml_op_name(_nodes(rt, _sum_rows)["r"]["op"]) == b"SUM_ROWS"
    assert rt.ggml_op_name(_nodes(rt, _argsort(DESC))["r"]["op"]) == b"ARGSORT"


@pytest.mark.parametrize("case", list(CASES))
def test_node_shape(case):
    d = _nodes(G.runtime(), CASES[case])
    r = d["r"]
    if case.startswith("argsort"):
        assert r["type"] == I32 and r["ne"] == (60, 3, 2, 1) and r["nb"] == (4, 240, 720, 1440)
        assert r["op_params"][0] == (DESC if case.endswith("desc") else ASC) and r["src"][0] == "a" and r["view_src"] is None
    elif case == "top_k":
        assert r["type"] == I32 and r["ne"] == (2, 5, 1, 1) and r["nb"] == (4, 32, 160, 160)
        assert r["view_src"] == "argsort" and r["view_offs"] == 0 and r["src"][0] == "argsort"
        s = d["argsort"]
        assert s["ne"] == (8, 5, 1, 1) and s["op_params"][0] == DESC and s["src"][0] == "probs"
    elif case == "sum_rows":
        assert r["type"] == F32 and r["ne"] == (1, 3, 2, 2) and r["nb"] == (4, 4, 12, 24) and r["src"][0] == "a"
    else:
        assert r["type"] == F32 and r["ne"] == (2, 5, 1, 1) and r["src"][:3] == ["a", "b", None]
    assert not r["grad"]


@needs_ref
@pytest.mark.parametrize("case", list(CASES))
def test_node_equals_reference(case):
    ref = G.Lib([REF_LIB], isolated=True)
    ours, theirs = _nodes(G.runtime(), CASES[case]), _nodes(ref, CASES[case])
    assert ours == theirs
    assert ours["r"]["op"] != 0
