"""The half-precision Kronecker product's tune key on the host (no GPU): "bsr.kron_half" is 0 by
default (create_kron_bsr keeps refusing float16 / complex32), can be set to 1 and back, and an
unknown sibling key still fails.  The product is checked by tests/test_gpu_kron_half.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys
sys.path.insert(0, %r)
import superbblas_amd as sb
out = [sb.tune_get("bsr.kron_half")]
sb.tune_set("bsr.kron_half", 1)
out.append(sb.tune_get("bsr.kron_half"))
out.append(sb.tune_get("bsr.kron_mixed"))
sb.tune_set("bsr.kron_half", 0)
out.append(sb.tune_get("bsr.kron_half"))
for call in (lambda: sb.tune_get("bsr.kron_half_"), lambda: sb.tune_set("bsr.kron_half_", 1)):
    try:
        call()
        out.append("accepted")
    except sb.SuperbblasError:
        out.append("refused")
print(*out)
""" % ROOT


def test_kron_half_key_in_a_fresh_process():
    """a freshly loaded library (its own process: other tests of this one may have set the key);
    setting the key leaves bsr.kron_mixed at its 0"""
    out = subprocess.run([sys.executable, "-c", CODE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "1", "0", "0", "refused", "refused"]
