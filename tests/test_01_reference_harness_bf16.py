"""The reference's own conformance executable on the bf16 cases of GGML_OP_GET_ROWS and GGML_OP_CPY
(tests/test-backend-ops.cpp), compared op by op against the reference CPU backend: every such case runs and
passes, none is refused.

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

BF16 = re.compile(r"\bbf16\b")


@pytest.mark.parametrize("op", ["GET_ROWS", "CPY"])
def test_reference_backend_ops_bf16(op):
    env = dict(os.environ, GGML_MI355X_AUTOREGISTER="1")
    p = subprocess.run([OPS, "test", "-o", op, "-b", "MI355X0"], env=env, capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    lines = re.sub(r"\x1b\[[0-9;]*m", "", out).splitlines()
    bad = [ln for ln in lines if "FAIL" in ln]
    bf16 = [ln for ln in lines if BF16.search(ln)]
    refused = [ln for ln in bf16 if "not supported" in ln]
    print(f"{op}: {len(bf16)} bf16 lines, {len(bad)} FAIL in all, {len(refused)} refused")
    print("\n".join((bad + refused)[:40]))
    assert "Backend name: MI355X0" in out, out[-2000:]
    assert p.returncode == 0 and not bad, "\n".join(bad[:40]) or out[-3000:]
    assert not refused, "\n".join(refused[:40])
    assert bf16 and all(ln.rstrip().endswith("OK") for ln in bf16), "\n".join(ln for ln in bf16 if not ln.rstrip().endswith("OK"))
