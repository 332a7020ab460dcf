"""The Hermitian-output GEMM mode's tune keys on the host (no GPU): "gemm.herm" is off by default
(a mirrored imaginary part is the exact conjugate of its partner, not the bits of the full
product, so the mode is opt-in), can be set and read back, and the read-back "gemm.last_herm"
(tiles the last GEMM launch mirrored instead of computed) is 0 before any launch.  The kernels are
checked by tests/test_gpu_gemm_herm.py."""
import os
import subprocess
import sys

import pytest

import superbblas_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fresh_load_defaults():
    """a freshly loaded library (its own process: other tests of this one may have launched GEMMs):
    the mode off, nothing mirrored"""
    code = ("import sys; sys.path.insert(0, %r); import superbblas_amd as sb; "
            "print(sb.tune_get('gemm.herm'), sb.tune_get('gemm.last_herm'))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "0"]


def test_herm_settable():
    old = sb.tune_get("gemm.herm")
    sb.tune_set("gemm.herm", 1)
    try:
        assert sb.tune_get("gemm.herm") == 1
    finally:
        sb.tune_set("gemm.herm", old)
    assert sb.tune_get("gemm.herm") == old


def test_last_herm_is_read_only():
    assert sb.tune_get("gemm.last_herm") >= 0
    with pytest.raises(sb.SuperbblasError):
        sb.tune_set("gemm.last_herm", 1)
