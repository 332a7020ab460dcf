"""The lean GEMM main loop's tune keys on the host (no GPU): "gemm.lean" is on by default (the
lean form gives the generic kernel's bits), can be set and read back, and the read-back
"gemm.last_lean" is 0 before any launch and cannot be set.  The kernel is checked by
tests/test_gpu_gemm_lean.py."""
import os
import subprocess
import sys

import pytest

import superbblas_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fresh_load_defaults():
    """a freshly loaded library (its own process: other tests of this one may have launched GEMMs)"""
    code = ("import sys; sys.path.insert(0, %r); import superbblas_amd as sb; "
            "print(sb.tune_get('gemm.lean'), sb.tune_get('gemm.last_lean'))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "0"]


def test_lean_settable():
    old = sb.tune_get("gemm.lean")
    sb.tune_set("gemm.lean", 0)
    try:
        assert sb.tune_get("gemm.lean") == 0
    finally:
        sb.tune_set("gemm.lean", old)
    assert sb.tune_get("gemm.lean") == old


def test_last_lean_is_read_only():
    assert sb.tune_get("gemm.last_lean") in (0, 1)
    with pytest.raises(sb.SuperbblasError):
        sb.tune_set("gemm.last_lean", 1)
