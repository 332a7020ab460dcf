"""The in-place adjoint's tune keys on the host (no GPU): "bsr.adj_inplace" is 0 by default and
can be set and read back, the read-back "bsr.adj_copy_bytes" reads 0 before any operator exists
and cannot be set.  The product is checked by tests/test_gpu_bsr_adjoint_inplace.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys
sys.path.insert(0, %r)
import superbblas_amd as sb
out = [sb.tune_get("bsr.adj_inplace"), sb.tune_get("bsr.adj_copy_bytes")]
sb.tune_set("bsr.adj_inplace", 1)
out.append(sb.tune_get("bsr.adj_inplace"))
sb.tune_set("bsr.adj_inplace", 0)
out.append(sb.tune_get("bsr.adj_inplace"))
for call in (lambda: sb.tune_set("bsr.adj_copy_bytes", 0), lambda: sb.tune_get("bsr.adj_inplace_"),
             lambda: sb.tune_set("bsr.adj_inplace_", 1)):
    try:
        call()
        out.append("accepted")
    except sb.SuperbblasError:
        out.append("refused")
out.append(sb.tune_get("bsr.adj_copy_bytes"))
print(*out)
""" % ROOT


def test_adjoint_inplace_keys_in_a_fresh_process():
    """a freshly loaded library (its own process: other tests of this one may have set the keys)"""
    out = subprocess.run([sys.executable, "-c", CODE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "0", "1", "0", "refused", "refused", "refused", "0"]
