"""Half-precision Kronecker operators through the drop-in C++ header:
tests/cpp/kron_half_test.cpp calls create_kron_bsr<6, 6, superbblas::complex_float16> -- refused
with "bsr.kron_half" at 0 -- and then, with the key at 1 (set through sbx_tune_set),
bsr_krylov<6, 6, 8, 8, std::complex<float>> on that handle: A x and A^H x exact against host loops
in double; a std::complex<double> call stays refused and leaves y untouched.
Compiled here with plain g++, by the command of tests/cpp/Makefile."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_kron_half_dropin_application(gpu):
    cpp = os.path.join(HERE, "cpp")
    src, exe = os.path.join(cpp, "kron_half_test.cpp"), os.path.join(cpp, "kron_half_test")
    lib = os.path.join(ROOT, "superbblas_amd", "libsuperbblas_amd.so")
    hdr = os.path.join(ROOT, "include", "superbblas.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(lib),
                                                              os.path.getmtime(hdr)):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-Wall",
                               "-I" + os.path.join(ROOT, "include"), src,
                               "-L" + os.path.join(ROOT, "superbblas_amd"), "-lsuperbblas_amd",
                               "-Wl,-rpath,$ORIGIN/../../superbblas_amd", "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kron_half_test: all checks passed" in r.stdout, (r.stdout, r.stderr)
