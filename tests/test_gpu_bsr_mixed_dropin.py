"""Mixed-precision bsr_krylov through the drop-in C++ header: tests/cpp/mixed_bsr_test.cpp calls
create_bsr<6, 6, std::complex<float>> and then bsr_krylov<6, 6, 8, 8, std::complex<double>> on
that handle, compares with a host loop in double, and checks that the reverse pair throws
std::runtime_error.  Compiled here with plain g++, by the command of tests/cpp/Makefile."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_mixed_dropin_application(gpu):
    cpp = os.path.join(HERE, "cpp")
    src, exe = os.path.join(cpp, "mixed_bsr_test.cpp"), os.path.join(cpp, "mixed_bsr_test")
    lib = os.path.join(ROOT, "superbblas_amd", "libsuperbblas_amd.so")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(lib)):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-Wall",
                               "-I" + os.path.join(ROOT, "include"), src,
                               "-L" + os.path.join(ROOT, "superbblas_amd"), "-lsuperbblas_amd",
                               "-Wl,-rpath,$ORIGIN/../../superbblas_amd", "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mixed_bsr_test: all checks passed" in r.stdout, (r.stdout, r.stderr)
