"""The tune keys of the 12x12 mixed-precision BSR kernels on the host (no GPU):
"bsr.mixed12_min_cols" is 4 and "bsr.mixed12_pack" 1 in a freshly loaded library, both can be set
and read back, and an unknown sibling key still fails.  The products are checked by
tests/test_gpu_bsr_mixed12.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys
sys.path.insert(0, %r)
import superbblas_amd as sb
out = [sb.tune_get("bsr.mixed12_min_cols")]
for v in (1, 12, 4):
    sb.tune_set("bsr.mixed12_min_cols", v)
    out.append(sb.tune_get("bsr.mixed12_min_cols"))
out.append(sb.tune_get("bsr.mixed12_pack"))
for v in (0, 2, 1):
    sb.tune_set("bsr.mixed12_pack", v)
    out.append(sb.tune_get("bsr.mixed12_pack"))
for call in (lambda: sb.tune_get("bsr.mixed12_min_col"), lambda: sb.tune_set("bsr.mixed12_min_col", 1)):
    try:
        call()
        out.append("accepted")
    except sb.SuperbblasError:
        out.append("refused")
print(*out)
""" % ROOT


def test_mixed12_keys_in_a_fresh_process():
    """a freshly loaded library (its own process: other tests of this one may have set the key)"""
    out = subprocess.run([sys.executable, "-c", CODE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["4", "1", "12", "4", "1", "0", "2", "1", "refused", "refused"]
