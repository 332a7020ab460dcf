"""Half-precision BSR operator values, the parts that need no GPU: the binding's enum values and
the drop-in header's storage-only types superbblas::float16 / complex_float16 (sizes 2 and 4,
trivially copyable, mapped to SBX_HALF / SBX_CHALF), with create_bsr and both bsr_krylov overloads
instantiated on them -- plain g++, no _Float16 needed -- also against the declarations-only
<mpi.h> with SUPERBBLAS_USE_MPI."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "half_bsr_compile.cpp")


def test_binding_enum_values():
    import torch
    import superbblas_amd as sb
    assert sb.HALF == 6 and sb.CHALF == 7
    assert sb._DTYPES[torch.float16] == sb.HALF and sb._DTYPES[torch.complex32] == sb.CHALF
    # the tensor types keep their values
    assert (sb.FLOAT, sb.DOUBLE, sb.CFLOAT, sb.CDOUBLE, sb.INT, sb.SIZE_T) == tuple(range(6))


@pytest.mark.parametrize("std", ["-std=c++14", "-std=c++17"])
@pytest.mark.parametrize("mpi", [False, True])
def test_header_half_types_compile(std, mpi):
    args = ["g++", std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    if mpi:
        args += ["-DSUPERBBLAS_USE_MPI", "-I", os.path.join(ROOT, "tests", "cpp", "mpi_stub")]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(args + ["-c", SRC, "-o", os.path.join(d, "t.o")], capture_output=True,
                           text=True)
    assert r.returncode == 0, r.stderr


def test_c_abi_enum_compiles_as_c():
    src = ('#include "superbblas_amd/sbx.h"\n'
           "typedef char half_is_6[SBX_HALF == 6 ? 1 : -1];\n"
           "typedef char chalf_is_7[SBX_CHALF == 7 ? 1 : -1];\n"
           "int main(void) { return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "t.c")
        with open(f, "w") as fh:
            fh.write(src)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-fsyntax-only", f], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
