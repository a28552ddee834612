"""tests/ops_cases.py on MI355X against the reference CPU library: forced sequential fallbacks of cpu_order.h in
k_norm and in the GEMV prologues, ggml_rope_custom over its parameter space, and the layouts, type pairs and
row lengths of the remaining companion ops. Identical bits everywhere, except RoPE positions outside the
backend's table (ops_cases.rope_bound). A forced/ or rope/ case also asserts the backend's launch count, which
proves the route: k_norm alone, the one fused GEMV launch, one launch per ROPE node.

tests/test_ops_cases.py proves on the CPU that the forced rows are forced and distinguishable; DESIGN.md
section 4.9 lists which case fails when a fallback is broken."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from ggml_mi355x import ggml as G
import ops_cases as OC

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")]


@pytest.fixture(scope="module")
def libs():
    # one backend for the module: it keeps a RoPE table per parameter set for its life
    rt = G.runtime()
    be = G.mi355x_backend(rt)
    ref = G.Lib([REF_LIB], isolated=True)
    cpu = ref.ggml_backend_cpu_init()
    yield rt, be, ref, cpu
    ref.ggml_backend_free(cpu)
    rt.ggml_backend_free(be)


_reference = {}


def reference(libs, cs):
    """What the case must give, computed once and left unchanged: the reference CPU's outputs, or numpy's for
    the element-wise type pairs the reference CPU aborts on."""
    if cs.name not in _reference:
        _, _, ref, cpu = libs
        outs = cs.expect() if cs.expect is not None else OC.run_case(ref, cpu, cs, True)[0]
        for v in outs.values():
            v.setflags(write=False)
        _reference[cs.name] = outs
    return _reference[cs.name]


def graph_stats(rt, be):
    arr = (ctypes.c_int64 * 6)()
    assert rt.ggml_backend_mi355x_graph_stats_ex(be, arr, 6) == 6
    return list(arr)


def check(libs, cs):
    rt, be, _, _ = libs
    want = reference(libs, cs)
    for order in cs.orders:
        s0 = graph_stats(rt, be)
        if order is not None:
            assert rt.ggml_backend_mi355x_set_tuning(b"mmv_order", order)
        try:
            got, n_launch = OC.run_case(rt, be, cs, False)
        finally:
            if order is not None:
                rt.ggml_backend_mi355x_set_tuning(b"mmv_order", -1)
        s1 = graph_stats(rt, be)
        print(f"{cs} mmv_order={order}: {n_launch} launches")
        assert got.keys() == want.keys()
        failed = []
        for name in want:
            a, b = got[name], want[name]
            assert a.dtype == b.dtype and a.shape == b.shape
            if cs.check is not None:
                failed += cs.check(name, a, b)
            elif not OC.same_bits(a, b):
                failed.append(f"{name}: {int(np.sum(a.view(np.uint8) != b.view(np.uint8)))}/{a.nbytes} bytes differ (identical bits expected)")
        assert not failed, failed
        if cs.launches is not None:
            assert n_launch == cs.launches, (n_launch, cs.launches)
        if cs.replays:
            # the backend's counters: [3] direct computes, [4] replays of a cached capture, [5] captures. The first compute
            # of the graph runs directly, the second is captured, the rest replay it
            print(f"{cs}: graph stats {s0} -> {s1}")
            assert s1[5] - s0[5] >= 1 and s1[4] - s0[4] >= 1, (s0, s1)


@pytest.mark.parametrize("cs", OC.by_prefix("forced/k_norm/"), ids=repr)
def test_forced_fallback_in_k_norm(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("forced/f16-"), ids=repr)
def test_forced_fallback_in_f16_gemv_prologue(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("forced/q-prologue/"), ids=repr)
def test_forced_fallback_in_quantized_gemv_prologue(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("forced/q-prologue1/"), ids=repr)
def test_forced_fallback_in_single_column_q8k_prologue(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("rope/"), ids=repr)
def test_rope_custom(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", [c for op in ("add", "sub", "mul", "div") for c in OC.by_prefix(f"layout/{op}/")], ids=repr)
def test_binary_layouts_and_type_pairs(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", [c for op in ("scale", "gelu", "silu") for c in OC.by_prefix(f"layout/{op}/")], ids=repr)
def test_unary_layouts(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", [c for op in ("cpy", "cont", "dup") for c in OC.by_prefix(f"layout/{op}/")], ids=repr)
def test_copy_layouts_and_quantized_destinations(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("layout/diag_mask"), ids=repr)
def test_diag_mask(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("layout/norm/") + OC.by_prefix("layout/rms_norm/"), ids=repr)
def test_norm_row_lengths_and_layouts(libs, cs):
    check(libs, cs)


@pytest.mark.parametrize("cs", OC.by_prefix("layout/soft_max/"), ids=repr)
def test_soft_max_row_lengths_masks_and_layouts(libs, cs):
    check(libs, cs)


def test_every_case_runs():
    """No case of the table is left out of the tests above."""
    ran = set()
    for p in ("forced/k_norm/", "forced/f16-", "forced/q-prologue/", "forced/q-prologue1/", "rope/", "layout/"):
        ran |= {c.name for c in OC.by_prefix(p)}
    layout = {c.name.split("/")[1] for c in OC.by_prefix("layout/")}
    assert ran == set(OC.BY_NAME)
    assert layout == {"add", "sub", "mul", "div", "scale", "gelu", "silu", "cpy", "cont", "dup", "diag_mask_inf", "diag_mask_zero",
                      "norm", "rms_norm", "soft_max"}
