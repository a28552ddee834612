"""The reference's own conformance executable on the router ops GGML_OP_ARGSORT and GGML_OP_SUM_ROWS
(tests/test-backend-ops.cpp test_argsort: [8, 1, 1, 1], [16, 10, 10, 10] and [60, 10, 10, 10] rows in
both orders; test_sum_rows), compared op by op against the reference CPU backend (NMSE <= 5e-4).

Named test_01_* so it runs, as test_00_reference_harness.py, before any test initialises HIP in the
pytest process (the harness is a child process).
"""
import os
import re
import subprocess

import pytest

from conftest import REPO

OPS = os.path.join(REPO, "oracle", "_ref", "test-backend-ops-mi355x")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(OPS), reason="harness not built (make -C oracle harness)")]


def _run(op):
    env = dict(os.environ, GGML_MI355X_AUTOREGISTER="1")
    p = subprocess.run([OPS, "test", "-o", op, "-b", "MI355X0"], env=env, capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    lines = re.sub(r"\x1b\[[0-9;]*m", "", out).splitlines()
    bad = [ln for ln in lines if "FAIL" in ln]
    ok = [ln for ln in lines if ln.rstrip().endswith("OK")]
    refused = [ln for ln in lines if "not supported" in ln]
    print(f"{op}: {len(ok)} OK, {len(bad)} FAIL, {len(refused)} refused")
    print("\n".join((bad + refused)[:40]))
    assert "Backend name: MI355X0" in out, out[-2000:]
    assert p.returncode == 0 and not bad, "\n".join(bad[:40]) or out[-3000:]
    assert not refused, "\n".join(refused[:40])
    return ok


def test_reference_backend_ops_argsort():
    assert len(_run("ARGSORT")) >= 6


def test_reference_backend_ops_sum_rows():
    assert len(_run("SUM_ROWS")) >= 1
