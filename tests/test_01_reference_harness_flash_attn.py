"""The reference's own conformance executable on GGML_OP_FLASH_ATTN_EXT (tests/test-backend-ops.cpp
test_flash_attn_ext: head sizes 64 / 80 / 128 / 256, 32 heads, 512 and 1024 keys, 1 / 2 / 4 / 8 queries,
with and without mask and ALiBi -- 96 cases), compared against the reference CPU backend at the
harness's own NMSE <= 5e-4.

Named test_01_* so it runs, as test_00_reference_harness.py, before any test initialises HIP in the
pytest process (the harness is a child process).
"""
import os

import pytest

from conftest import REPO
from test_01_reference_harness_router import _run

OPS = os.path.join(REPO, "oracle", "_ref", "test-backend-ops-mi355x")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(OPS), reason="harness not built (make -C oracle harness)")]


def test_reference_backend_ops_flash_attn_ext():
    ok = [ln for ln in _run("FLASH_ATTN_EXT") if "FLASH_ATTN_EXT" in ln]
    assert len(ok) == 96, len(ok)
