// Compile-only check of the half-precision value types of include/superbblas.h (-fsyntax-only,
// with and without SUPERBBLAS_USE_MPI against tests/cpp/mpi_stub; see tests/test_cpu_bsr_half.py):
// create_bsr with superbblas::float16 and superbblas::complex_float16 values, and bsr_krylov in
// float and std::complex<float> on such handles.
#include "superbblas.h"

#include <type_traits>

using namespace superbblas;
using C = std::complex<float>;

static_assert(sizeof(float16) == 2 && alignof(float16) == 2, "binary16: 16 bits");
static_assert(sizeof(complex_float16) == 4 && alignof(complex_float16) == 2, "two binary16: re, im");
static_assert(std::is_trivially_copyable<float16>::value &&
                  std::is_trivially_copyable<complex_float16>::value &&
                  std::is_standard_layout<float16>::value &&
                  std::is_standard_layout<complex_float16>::value,
              "storage-only types");
static_assert(sbx_detail::dtype<float16>::value == SBX_HALF && SBX_HALF == 6 &&
                  sbx_detail::dtype<complex_float16>::value == SBX_CHALF && SBX_CHALF == 7,
              "the C ABI's enum values");
#ifdef __FLT16_MANT_DIG__
static_assert(sbx_detail::dtype<_Float16>::value == SBX_HALF, "_Float16 where the compiler has it");
#endif

template <typename V, typename T> void use_half(
#ifdef SUPERBBLAS_USE_MPI
    MPI_Comm comm
#endif
) {
    Context gpu = createGpuContext(0);
    const Coor<2> d{4, 4};
    PartitionItem<2> p{Coor<2>{}, d};
    IndexType *ii = nullptr;
    Coor<2> *jj = nullptr;
    const V *v = nullptr;
    BSR_handle *op = nullptr;
    const T *x = nullptr;
    T *y = nullptr;
    const PartitionItem<3> px{Coor<3>{}, Coor<3>{4, 4, 2}};
#ifdef SUPERBBLAS_USE_MPI
    create_bsr<2, 2, V>(&p, d, &p, d, 1, Coor<2>{1, 1}, Coor<2>{1, 1}, false, &ii, &jj, &v, &gpu,
                        comm, SlowToFast, &op);
    bsr_krylov<2, 2, 3, 3, T>(T(1), op, "ab", "AB", &px, 1, "ABn", Coor<3>{}, Coor<3>{4, 4, 2},
                              Coor<3>{4, 4, 2}, &x, T(0), &px, "abn", Coor<3>{}, Coor<3>{4, 4, 2},
                              Coor<3>{4, 4, 2}, 0, &y, &gpu, comm, SlowToFast);
#endif
    create_bsr<2, 2, V>(&p, d, &p, d, 1, Coor<2>{1, 1}, Coor<2>{1, 1}, false, &ii, &jj, &v, &gpu,
                        SlowToFast, &op);
    bsr_krylov<2, 2, 3, 3, T>(T(1), op, "ab", "AB", &px, 1, "ABn", Coor<3>{}, Coor<3>{4, 4, 2},
                              Coor<3>{4, 4, 2}, &x, T(0), &px, "abn", Coor<3>{}, Coor<3>{4, 4, 2},
                              Coor<3>{4, 4, 2}, 0, &y, &gpu, SlowToFast);
    destroy_bsr(op);
}

#ifdef SUPERBBLAS_USE_MPI
template void use_half<float16, float>(MPI_Comm);
template void use_half<complex_float16, C>(MPI_Comm);
#else
template void use_half<float16, float>();
template void use_half<complex_float16, C>();
#endif
