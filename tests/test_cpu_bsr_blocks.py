"""The dense-block BSR kernel's tune keys on the host (no GPU): "bsr.blk_mfma" is on by default,
"bsr.blk_min" is 16, both can be set and read back, and the read-back "bsr.last_kernel" cannot be
set.  The kernel is checked by tests/test_gpu_bsr_blocks.py."""
import os
import subprocess
import sys

import pytest

import superbblas_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fresh_load_defaults():
    """a freshly loaded library (its own process: other tests of this one may have set the keys)"""
    code = ("import sys; sys.path.insert(0, %r); import superbblas_amd as sb; "
            "print(sb.tune_get('bsr.blk_mfma'), sb.tune_get('bsr.blk_min'))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "16"]


@pytest.mark.parametrize("key,value", [("bsr.blk_mfma", 0), ("bsr.blk_min", 4)])
def test_keys_settable(key, value):
    old = sb.tune_get(key)
    sb.tune_set(key, value)
    try:
        assert sb.tune_get(key) == value
    finally:
        sb.tune_set(key, old)
    assert sb.tune_get(key) == old


def test_last_kernel_is_read_only():
    assert sb.tune_get("bsr.last_kernel") >= 0
    with pytest.raises(sb.SuperbblasError):
        sb.tune_set("bsr.last_kernel", 14)
