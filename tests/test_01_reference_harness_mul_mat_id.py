"""The reference's own conformance executable on GGML_OP_MUL_MAT_ID (tests/test-backend-ops.cpp
test_mul_mat_id: every weight type, 4 / 8 experts, 1 / 2 / 4 used, b broadcast or not, 1 / 32 tokens,
ids a strided view), compared op by op against the reference CPU backend (NMSE <= 5e-4).

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

SUPPORTED = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q4_K", "q5_K", "q6_K", "f16", "f32")


def test_reference_backend_ops_mul_mat_id():
    env = dict(os.environ, GGML_MI355X_AUTOREGISTER="1")
    p = subprocess.run([OPS, "test", "-o", "MUL_MAT_ID", "-b", "MI355X0"], env=env, capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    lines = re.sub(r"\x1b\[[0-9;]*m", "", out).splitlines()
    bad = [ln for ln in lines if "FAIL" in ln]
    ok = [ln for ln in lines if ln.rstrip().endswith("OK")]
    refused = [ln for ln in lines if "not supported" in ln and re.search(r"type_a=(%s)," % "|".join(SUPPORTED), ln)]
    print(f"MUL_MAT_ID: {len(ok)} OK, {len(bad)} FAIL, {len(refused)} supported-type cases refused")
    print("\n".join((bad + refused)[:40]))
    assert "Backend name: MI355X0" in out, out[-2000:]
    assert p.returncode == 0 and not bad, "\n".join(bad[:40]) or out[-3000:]
    assert ok, "no MUL_MAT_ID case ran on MI355X0"
    assert not refused, "\n".join(refused[:40])
