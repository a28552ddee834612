"""tests/fusion_cases.py on the reference CPU library alone: every case builds and computes, its absorbable
operands move the output they are pinned by, and no node's destination partially overlaps its own sources
(which would leave the oracle undefined as well). The same cases run on MI355X in tests/test_fusion_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
import fusion_cases as FC

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")

pytestmark = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")

F32_EPS = 2.0 ** -23  # the comparison's resolution where the bound is identical bits


@pytest.fixture(scope="module")
def ref():
    lib = G.Lib([REF_LIB], isolated=True)
    cpu = lib.ggml_backend_cpu_init()
    yield lib, cpu
    lib.ggml_backend_free(cpu)


def partial_overlaps(L, g):
    """(node, source) pairs whose byte ranges overlap without being the same elements."""
    bad = []
    for t in FC.graph_nodes(g):
        n = t.contents
        if FC.op_name(L, t) in FC.NOOP_OPS or not n.data:
            continue
        lo, hi = n.data, n.data + L.ggml_nbytes(t)
        for k in range(10):
            if not n.src[k]:
                continue
            st = ctypes.cast(n.src[k], G.T)
            s = st.contents
            if not s.data or not (lo < s.data + L.ggml_nbytes(st) and s.data < hi):
                continue
            if s.data == n.data and list(s.ne) == list(n.ne) and list(s.nb) == list(n.nb):
                continue
            bad.append((n.name.decode() or FC.op_name(L, t), k))
    return bad


@pytest.mark.parametrize("cs", FC.CASES, ids=repr)
def test_case_on_reference_cpu(ref, cs):
    L, cpu = ref
    full, n_nodes, _, bad = FC.run_case(L, cpu, cs, inspect=partial_overlaps)
    assert "out" in full and n_nodes >= 1
    assert bad == [], f"destination partially overlaps a source: {bad}"
    if cs.positive:
        assert 0 <= min(cs.absorbed(o) for o in cs.orders) and max(cs.absorbed(o) for o in cs.orders) < n_nodes
    for name, v in full.items():
        ok = cs.masks.get(name, slice(None))
        assert not np.isnan(v[ok].astype(np.float32)).any(), f"{name} holds NaN"
    for operand, out in cs.absorbable.items():
        tol = max(cs.tol(out), F32_EPS)
        dropped = FC.run_case(L, cpu, cs, drop=operand)[0][out]
        a, b = full[out].astype(np.float64), dropped.astype(np.float64)
        fin = np.isfinite(a) & np.isfinite(b)
        moved = float(np.abs(a[fin] - b[fin]).max() / np.abs(a[fin]).max())
        print(f"{cs}: without {operand}, {out} moves by {moved:.3g} of max |{out}| (needs {100 * tol:.3g})")
        assert moved >= 100 * tol, (operand, out, moved)


def test_the_table_covers_every_pass():
    for prefix in ("norm/", "prologue/", "softmax/", "epilogue/", "copies/", "embedding/", "attention/"):
        assert FC.by_prefix(prefix, True) and FC.by_prefix(prefix, False), prefix
    assert all(name in FC.BY_NAME and FC.BY_NAME[name].positive for name in FC.GALLOCR)
