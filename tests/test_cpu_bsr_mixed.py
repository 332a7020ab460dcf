"""The mixed-precision BSR product's tune keys on the host (no GPU): "bsr.mixed" is 1 by default
and can be set and read back, the read-back "bsr.last_mixed" reads 0 before any launch, and an
unknown sibling key still fails.  The product is checked by tests/test_gpu_bsr_mixed.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys
sys.path.insert(0, %r)
import superbblas_amd as sb
out = [sb.tune_get("bsr.mixed"), sb.tune_get("bsr.last_mixed")]
sb.tune_set("bsr.mixed", 0)
out.append(sb.tune_get("bsr.mixed"))
sb.tune_set("bsr.mixed", 1)
out.append(sb.tune_get("bsr.mixed"))
for call in (lambda: sb.tune_get("bsr.mixed_"), lambda: sb.tune_set("bsr.mixed_", 1),
             lambda: sb.tune_set("bsr.last_mixed", 1)):
    try:
        call()
        out.append("accepted")
    except sb.SuperbblasError:
        out.append("refused")
print(*out)
""" % ROOT


def test_mixed_keys_in_a_fresh_process():
    """a freshly loaded library (its own process: other tests of this one may have set the keys)"""
    out = subprocess.run([sys.executable, "-c", CODE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "0", "0", "1", "refused", "refused", "refused"]
