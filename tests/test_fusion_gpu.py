"""The fusion passes' legality conditions on MI355X (tests/fusion_cases.py): every case runs on the backend and
on the reference CPU library, and every tensor the graph materialises is compared -- identical bits with
mmv_order 1, the project's tree-order tolerances with mmv_order 0. A positive case also asserts the backend's
launch count, which proves that the fused path is the one under test; a near-miss prints it.

A failure names the guard: the case ids are listed per pass and legality condition in DESIGN.md section 4.8."""
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
import fusion_cases as FC

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]


@pytest.fixture(scope="module")
def libs():
    rt = G.runtime()
    be = G.mi355x_backend(rt)
    ref = G.Lib([REF_LIB], isolated=True)
    cpu = ref.ggml_backend_cpu_init()
    yield rt, be, ref, cpu
    ref.ggml_backend_free(cpu)
    rt.ggml_backend_free(be)


_reference = {}


def reference(libs, cs):
    """The reference CPU's outputs of a case, computed once and left unchanged."""
    if cs.name not in _reference:
        _, _, ref, cpu = libs
        outs = FC.run_case(ref, cpu, cs)[0]
        for v in outs.values():
            v.setflags(write=False)
        _reference[cs.name] = outs
    return _reference[cs.name]


def in_order(rt, order, fn):
    assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
    try:
        return fn()
    finally:
        rt.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)


def compare(cs, order, got, want):
    assert got.keys() == want.keys()
    failed = []
    for name in want:
        ok = cs.masks.get(name, slice(None))
        a, b = got[name][ok], want[name][ok]
        tol = FC.EXACT if order == 1 else cs.tol(name)
        if FC.same_bits(a, b):
            continue
        fin = np.isfinite(b.astype(np.float32))
        if tol == FC.EXACT or not np.array_equal(np.isfinite(a.astype(np.float32)), fin):
            print(f"{cs} mmv_order={order}: {name} differs in {int(np.sum(a != b))}/{a.size} elements (identical bits expected)")
            failed.append(name)
            continue
        err = FC.rel_err(a[fin], b[fin])
        print(f"{cs} mmv_order={order}: {name} rel err {err:.2e} (bound {tol:.0e})")
        if not err <= tol:
            failed.append(name)
    return failed


def check(libs, cs):
    rt, be, _, _ = libs
    want = reference(libs, cs)
    for order in cs.orders:
        got, n_nodes, n_launch, _ = in_order(rt, order, lambda: FC.run_case(rt, be, cs))
        print(f"{cs} mmv_order={order}: {n_launch} launches for {n_nodes} nodes")
        failed = compare(cs, order, got, want)
        assert not failed, f"mmv_order={order}: {failed} differ from the reference CPU"
        if cs.positive:
            assert n_launch == n_nodes - cs.absorbed(order), (order, n_launch, n_nodes, cs.absorbed(order))


@pytest.mark.parametrize("cs", FC.by_prefix("norm/"), ids=repr)
def test_norm_chain(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("prologue/"), ids=repr)
def test_norm_as_gemv_prologue(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("softmax/"), ids=repr)
def test_soft_max_chain(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("epilogue/"), ids=repr)
def test_gemv_epilogue(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("copies/"), ids=repr)
def test_copy_batching(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("embedding/"), ids=repr)
def test_embedding(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", FC.by_prefix("attention/"), ids=repr)
def test_attention_block(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("name", FC.GALLOCR)
def test_chain_in_a_graph_allocator_buffer(libs, name):
    """The compute tensors share one buffer laid out by ggml_gallocr, which reuses the memory of dead tensors.
    The runtime's allocator releases a tensor four nodes after its last reader, so only the attention block
    is long enough for reuse (its merged output lands on Q's source: plan_attention copies Q to scratch); the
    shorter chains run unaliased and pin values alone. The deterministic aliasing cases are epilogue/aliased/*
    and epilogue/near/cpy-over-*. The final value is compared with the reference run the ordinary way."""
    rt, be, _, _ = libs
    cs = FC.BY_NAME[name]
    want = reference(libs, cs)["out"]
    for order in cs.orders:
        got, n_launch, size = in_order(rt, order, lambda: FC.run_case_gallocr(rt, be, cs))
        print(f"{cs} mmv_order={order} under gallocr: {n_launch} launches, compute buffer {size} bytes")
        if order == 1 or cs.tol("out") == FC.EXACT:
            assert FC.same_bits(got, want), f"mmv_order={order}: {int(np.sum(got != want))}/{got.size} elements differ"
        else:
            err = FC.rel_err(got, want)
            print(f"  rel err {err:.2e} (bound {cs.tol('out'):.0e})")
            assert err <= cs.tol("out"), (order, err)
