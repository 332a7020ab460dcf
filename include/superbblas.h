/*
 * superbblas.h -- drop-in C++ API of superbblas_amd.
 *
 * Keeps the template signatures of the reference's public API (eromero-vlc/superbblas
 * include/superbblas.h and the headers it pulls in) so that application code that calls
 * superbblas::copy / contraction / create_bsr / bsr_krylov / ... recompiles unchanged against
 * this header and libsuperbblas_amd.so.  Every template flattens its compile-time ranks into the
 * runtime descriptors of the C ABI (include/superbblas_amd/sbx.h) and rethrows a failing status
 * as std::runtime_error carrying the library's message (reference platform.h:226-243).
 *
 * Differences from the reference (documented in INTEGRATION.md):
 *  - The distributed overloads take a `superbblas::Communicator` (an sbx_comm: RCCL over xGMI,
 *    or host-staged through a user all-to-all) where the reference takes an MPI_Comm.  With
 *    SUPERBBLAS_USE_MPI defined, MPI_Comm overloads are provided (RCCL when every rank drives
 *    its own GPU, else host staging over MPI_Alltoallv).
 *  - Masks (mask0/mask1) must select the same elements (as the reference requires); `session`
 *    must be 0.  `request` is deferred for distributed copy() and bsr_krylov() (the exchange
 *    is started; wait() finishes it), complete on return otherwise (as the reference's no-MPI
 *    overloads, dist.h:3601, 3730).
 */
#ifndef SUPERBBLAS_AMD_SUPERBBLAS_H
#define SUPERBBLAS_AMD_SUPERBBLAS_H

#include "superbblas_amd/sbx.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <ostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

// The library always drives AMD GPUs (HIP): callers' GPU sections compile in, as with a reference
// build configured for HIP (superbblas_flags.h)
#ifndef SUPERBBLAS_USE_HIP
#    define SUPERBBLAS_USE_HIP
#endif
#ifndef SUPERBBLAS_USE_GPU
#    define SUPERBBLAS_USE_GPU
#endif

#ifdef SUPERBBLAS_USE_MPI
#    include <map>
#    include <memory>
#    include <mpi.h>
#endif

namespace superbblas {

// ---- types (tensor.h:47-66, dist.h:39-61, platform.h:104-125, bsr.h:28-52) ----

using IndexType = int;
template <std::size_t Nd, typename Idx = IndexType> using Coor = std::array<Idx, Nd>;
template <std::size_t N> using PartitionItem = std::array<Coor<N>, 2>;
template <std::size_t N> using Order = std::array<char, N>;
using MaskType = float;
using Session = unsigned int;
using Request = std::function<void(void)>;

enum CoorOrder { SlowToFast, FastToSlow };
enum CopyAdd { Copy, Add };
enum MatrixLayout { RowMajor, ColumnMajor };
enum platform { CPU, CUDA, HIP };
constexpr int CPU_DEVICE_ID = -1;
const platform GPU = HIP;

namespace detail {
struct Cpu;
struct Hip;
} // namespace detail

class Context {
public:
    enum platform plat;
    int device;
    Context(enum platform plat, int device) : plat(plat), device(device) {}
    /// The low-level contexts of the superbblas::detail surface (platform.h:765-773)
    detail::Cpu toCpu(Session session) const;
    detail::Hip toGpu(Session session) const;
};

inline Context createCpuContext() { return Context{CPU, CPU_DEVICE_ID}; }
inline Context createHipContext(int device = 0) { return Context{HIP, device}; }
inline Context createGpuContext(int device = 0) { return Context{GPU, device}; }
inline Context createCudaContext(int) {
    throw std::runtime_error("createCudaContext: superbblas_amd runs on AMD GPUs only");
}

struct BSR_handle; // opaque (sbx_bsr)

/// Half-precision value types of create_bsr (an extension): IEEE binary16 and a complex of two
/// of them (re, im).  Storage only -- the bit patterns, trivially copyable, the layout of
/// _Float16 / __half / __half2 and of torch's float16 / complex32 -- with no arithmetic: the
/// library never computes in 16 bits on the host, and the header needs no compiler support for
/// the format.  Fill them from the bits of a conversion of your own (or from _Float16 where the
/// compiler has it: create_bsr<Nd, Ni, _Float16> maps to the same type).
struct float16 {
    std::uint16_t bits;
};
struct complex_float16 {
    float16 re, im;
};
static_assert(sizeof(float16) == 2 && sizeof(complex_float16) == 4, "binary16 layout");

/// supported_type<T>::value: whether T is an element type of the library (platform.h:686-712,
/// 818-821)
template <typename T> struct supported_type { static constexpr bool value = false; };
template <> struct supported_type<int> { static constexpr bool value = true; };
template <> struct supported_type<float> { static constexpr bool value = true; };
template <> struct supported_type<double> { static constexpr bool value = true; };
template <> struct supported_type<std::complex<float>> { static constexpr bool value = true; };
template <> struct supported_type<std::complex<double>> { static constexpr bool value = true; };
template <> struct supported_type<_Complex float> { static constexpr bool value = true; };
template <> struct supported_type<_Complex double> { static constexpr bool value = true; };
template <typename T> struct supported_type<const T> {
    static constexpr bool value = supported_type<T>::value;
};

// ---- runtime features: the reference's SB_* environment flags (runtime_features.h:15-158) ----
//
// The library reads the same variables itself (SB_TRACK_TIME turns its kernel timers on,
// SB_CACHEGB_GPU caps its scratch cache, SB_DEBUG adds syncs / barriers around copy and
// contraction, SB_LOG reports failed allocations), so Python and C callers see them too.  The
// functions returning a reference may be assigned at run time, as in the reference; a change of
// getTrackingTime() reaches the library on the next API call.

namespace sbx_detail {
/// The integer value of an environment variable, or `def` when unset
inline int env_int(const char *name, int def) {
    const char *l = std::getenv(name);
    return l ? std::atoi(l) : def;
}
inline double env_double(const char *name, double def) {
    const char *l = std::getenv(name);
    return l ? std::atof(l) : def;
}
} // namespace sbx_detail

/// SB_LOG: 0 no log (default), >= 1 some log
inline int getLogLevel() {
    static const int v = std::max(0, sbx_detail::env_int("SB_LOG", 0));
    return v;
}
/// SB_DEBUG: 0 no extra checks (default), >= 1 GPU sync and barriers around copy and contraction
inline int getDebugLevel() {
    static const int v = std::max(0, sbx_detail::env_int("SB_DEBUG", 0));
    return v;
}
/// SB_TRACK_MEM: != 0 tracks memory use (reportCacheUsage / checkForMemoryLeaks always report)
inline bool &getTrackingMemory() {
    static bool v = sbx_detail::env_int("SB_TRACK_MEM", 0) != 0;
    return v;
}
/// SB_TRACK_TIME: != 0 records the time of the library's kernels (reportTimings)
inline bool &getTrackingTime() {
    static bool v = sbx_detail::env_int("SB_TRACK_TIME", 0) != 0;
    return v;
}
/// SB_TRACK_TIME_SYNC: accepted; timings are HIP events on the launch stream, no sync needed
inline bool &getTrackingTimeSync() {
    static bool v = sbx_detail::env_int("SB_TRACK_TIME_SYNC", 0) != 0;
    return v;
}
/// SB_MPI_NONBLOCK (default on): exchanges are always asynchronous on the library's streams
inline bool getUseMPINonBlock() {
    static const bool v = sbx_detail::env_int("SB_MPI_NONBLOCK", 1) != 0;
    return v;
}
/// SB_USE_ALLTOALL (default on): RCCL exchanges are grouped send/recv either way
inline bool getUseAlltoall() {
    static const bool v = sbx_detail::env_int("SB_USE_ALLTOALL", 1) != 0;
    return v;
}
/// SB_MPI_GPU: 0 unset, 1 device buffers go straight to the transport (RCCL), -1 they are staged
/// through host memory (the MPI_Comm overloads' transport choice)
inline int getUseMPIGpu() {
    static const int v =
        std::getenv("SB_MPI_GPU") ? (sbx_detail::env_int("SB_MPI_GPU", 0) != 0 ? 1 : -1) : 0;
    return v;
}
/// SB_CACHEGB_CPU: accepted (host components are mirrored through device scratch)
inline double getMaxCacheGiBCpu() {
    static const double v = sbx_detail::env_double("SB_CACHEGB_CPU", -1.0);
    return v;
}
/// SB_CACHEGB_GPU: cap of the idle scratch cache per device in GiB (< 0: 10 % of the device)
inline double getMaxCacheGiBGpu() {
    static const double v = sbx_detail::env_double("SB_CACHEGB_GPU", -1.0);
    return v;
}

namespace sbx_detail {
/// Hand a run-time change of getTrackingTime() to the library (its timers start from the same
/// SB_TRACK_TIME value)
inline void sync_tracking() {
    static bool applied = getTrackingTime();
    if (applied != getTrackingTime()) {
        applied = getTrackingTime();
        (void)sbx_timings_enable(applied ? 1 : 0);
    }
}
} // namespace sbx_detail

/// elem<T>::type is T's element type if T is an array, otherwise T (blas.h:98-108)
template <typename T> struct elem { using type = T; };
template <typename T, std::size_t N> struct elem<std::array<T, N>> {
    using type = typename elem<T>::type;
};
template <typename T, std::size_t N> struct elem<const std::array<T, N>> {
    using type = typename elem<T>::type;
};

/// Communicator of the distributed overloads (replaces MPI_Comm)
using Communicator = sbx_comm;

inline void wait(const Request &request) {
    if (request) request();
}

namespace sbx_detail {

inline void check(int rc) {
    if (rc != SBX_OK) throw std::runtime_error(sbx_last_error());
}

/// A Request over a C-ABI handle (sbx_wait once; copies of the Request share the handle)
inline Request request_of(sbx_request h) {
    if (!h) return Request{};
    auto shared = std::make_shared<sbx_request>(h);
    return [shared]() {
        sbx_request r = *shared;
        *shared = nullptr;
        if (r) check(sbx_wait(r));
    };
}

template <typename T> struct dtype;
template <> struct dtype<float> { static constexpr int value = SBX_FLOAT; };
template <> struct dtype<double> { static constexpr int value = SBX_DOUBLE; };
template <> struct dtype<std::complex<float>> { static constexpr int value = SBX_CFLOAT; };
template <> struct dtype<std::complex<double>> { static constexpr int value = SBX_CDOUBLE; };
template <> struct dtype<int> { static constexpr int value = SBX_INT; };
template <> struct dtype<std::size_t> { static constexpr int value = SBX_SIZE_T; };
/// The half-precision value types of create_bsr (below); every other call refuses them
template <> struct dtype<float16> { static constexpr int value = SBX_HALF; };
template <> struct dtype<complex_float16> { static constexpr int value = SBX_CHALF; };
#ifdef __FLT16_MANT_DIG__
template <> struct dtype<_Float16> { static constexpr int value = SBX_HALF; };
#endif
/// char has no values type in the C ABI (the reference's own char save / load do not compile,
/// tensor.h:1091, no multiplication_cost<char>): -1 fails every library call on char tensors
/// loudly, while programs that only name the type (tests/storage_details.cpp's type switch over a
/// file's values_datatype) compile
template <> struct dtype<char> { static constexpr int value = -1; };

template <typename T> inline std::array<double, 2> scalar(const T &v) { return {{(double)v, 0.0}}; }
template <typename T> inline std::array<double, 2> scalar(const std::complex<T> &v) {
    return {{(double)v.real(), (double)v.imag()}};
}

inline std::vector<sbx_context> contexts(const Context *ctx, int n) {
    if (!ctx) throw std::runtime_error("null context array");
    std::vector<sbx_context> r(n);
    for (int i = 0; i < n; ++i) {
        r[i].plat = ctx[i].plat == CPU ? SBX_CPU : SBX_GPU;
        r[i].device = ctx[i].plat == CPU ? -1 : ctx[i].device;
    }
    return r;
}

template <std::size_t N> inline const int *parts(const PartitionItem<N> *p) {
    static_assert(sizeof(PartitionItem<N>) == 2 * N * sizeof(int), "PartitionItem layout");
    return reinterpret_cast<const int *>(p);
}

inline void check_session(Session s) {
    if (s != 0) throw std::runtime_error("superbblas_amd: session must be 0");
    sync_tracking(); // every entry point checks its session first
}

inline int co_of(CoorOrder co) { return co == SlowToFast ? SBX_SLOW_TO_FAST : SBX_FAST_TO_SLOW; }

template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void copy_impl(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
               const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0,
               const Coor<Nd0> &dim0, const T **v0, const MaskType **mask0, const Context *ctx0,
               const PartitionItem<Nd1> *p1, int ncomponents1, const char *o1,
               const Coor<Nd1> &from1, const Coor<Nd1> &dim1, Q **v1, const MaskType **mask1,
               const Context *ctx1, sbx_comm comm, CoorOrder co, CopyAdd copyadd,
               Request *request, Session session) {
    static_assert(std::is_same<MaskType, float>::value, "MaskType is float (tensor.h:54)");
    check_session(session);
    const auto a = scalar(alpha);
    const auto c0 = contexts(ctx0, ncomponents0), c1 = contexts(ctx1, ncomponents1);
    sbx_request h = nullptr;
    check(sbx_copy_req((int)Nd0, (int)Nd1, a.data(), dtype<T>::value, dtype<Q>::value,
                       parts(p0), ncomponents0, o0, from0.data(), size0.data(), dim0.data(),
                       (const void *const *)v0, (const float *const *)mask0, c0.data(),
                       parts(p1), ncomponents1, o1, from1.data(), dim1.data(),
                       (void *const *)v1, (const float *const *)mask1, c1.data(), comm,
                       co_of(co), copyadd == Copy ? SBX_COPY : SBX_ADD, 0,
                       request ? &h : nullptr));
    if (request) *request = request_of(h);
}

template <std::size_t Nd0, std::size_t Nd1, std::size_t Ndo, typename T>
void contraction_impl(T alpha, const PartitionItem<Nd0> *p0, const Coor<Nd0> &from0,
                      const Coor<Nd0> &size0, const Coor<Nd0> &dim0, int ncomponents0,
                      const char *o0, bool conj0, const T **v0, const Context *ctx0,
                      const PartitionItem<Nd1> *p1, const Coor<Nd1> &from1,
                      const Coor<Nd1> &size1, const Coor<Nd1> &dim1, int ncomponents1,
                      const char *o1, bool conj1, const T **v1, const Context *ctx1, T beta,
                      const PartitionItem<Ndo> *pr, const Coor<Ndo> &fromr,
                      const Coor<Ndo> &sizer, const Coor<Ndo> &dimr, int ncomponentsr,
                      const char *o_r, T **vr, const Context *ctxr, sbx_comm comm, CoorOrder co,
                      Request *request, Session session) {
    static_assert(!std::is_same<T, int>::value && !std::is_same<T, std::size_t>::value,
                  "contraction: unsupported type (dist.h:94-99)");
    check_session(session);
    const auto a = scalar(alpha), b = scalar(beta);
    const auto c0 = contexts(ctx0, ncomponents0), c1 = contexts(ctx1, ncomponents1),
               cr = contexts(ctxr, ncomponentsr);
    check(sbx_contraction((int)Nd0, (int)Nd1, (int)Ndo, dtype<T>::value, a.data(), parts(p0),
                          from0.data(), size0.data(), dim0.data(), ncomponents0, o0, conj0 ? 1 : 0,
                          (const void *const *)v0, c0.data(), parts(p1), from1.data(),
                          size1.data(), dim1.data(), ncomponents1, o1, conj1 ? 1 : 0,
                          (const void *const *)v1, c1.data(), b.data(), parts(pr), fromr.data(),
                          sizer.data(), dimr.data(), ncomponentsr, o_r, (void *const *)vr,
                          cr.data(), comm, co_of(co), 0));
    if (request) *request = Request{};
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_bsr_impl(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi,
                     const PartitionItem<Nd> *pdm, const Coor<Nd> &dimd, int ncomponents,
                     const Coor<Ni> &blockim, const Coor<Nd> &blockdm, bool blockImFast,
                     IndexType **ii, Coor<Nd> **jj, const T **v, const Context *ctx,
                     sbx_comm comm, CoorOrder co, BSR_handle **bsrh, Session session) {
    check_session(session);
    const auto c = contexts(ctx, ncomponents);
    std::vector<const int *> jjp(ncomponents);
    for (int i = 0; i < ncomponents; ++i) jjp[i] = reinterpret_cast<const int *>(jj[i]);
    sbx_bsr h = nullptr;
    check(sbx_create_bsr((int)Nd, (int)Ni, dtype<T>::value, parts(pim), dimi.data(), parts(pdm),
                         dimd.data(), ncomponents, blockim.data(), blockdm.data(),
                         blockImFast ? 1 : 0, (const int *const *)ii, jjp.data(),
                         (const void *const *)v, c.data(), comm, co_of(co), &h, 0));
    *bsrh = reinterpret_cast<BSR_handle *>(h);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_kron_bsr_impl(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi,
                          const PartitionItem<Nd> *pdm, const Coor<Nd> &dimd, int ncomponents,
                          const Coor<Ni> &blockim, const Coor<Nd> &blockdm,
                          const Coor<Ni> &kronim, const Coor<Nd> &krondm, bool blockImFast,
                          IndexType **ii, Coor<Nd> **jj, const T **v, const T **kronv,
                          const Context *ctx, sbx_comm comm, CoorOrder co, BSR_handle **bsrh,
                          Session session) {
    check_session(session);
    const auto c = contexts(ctx, ncomponents);
    std::vector<const int *> jjp(ncomponents);
    for (int i = 0; i < ncomponents; ++i) jjp[i] = reinterpret_cast<const int *>(jj[i]);
    sbx_bsr h = nullptr;
    check(sbx_create_kron_bsr((int)Nd, (int)Ni, dtype<T>::value, parts(pim), dimi.data(),
                              parts(pdm), dimd.data(), ncomponents, blockim.data(),
                              blockdm.data(), kronim.data(), krondm.data(), blockImFast ? 1 : 0,
                              (const int *const *)ii, jjp.data(), (const void *const *)v,
                              (const void *const *)kronv, c.data(), comm, co_of(co), &h, 0));
    *bsrh = reinterpret_cast<BSR_handle *>(h);
}

template <std::size_t Nd, std::size_t Ni, std::size_t Nx, std::size_t Ny, typename T>
void bsr_krylov_impl(T alpha, BSR_handle *bsrh, const char *oim, const char *odm,
                     const PartitionItem<Nx> *px, int ncomponents, const char *ox,
                     const Coor<Nx> &fromx, const Coor<Nx> &sizex, const Coor<Nx> &dimx,
                     const T **vx, T beta, const PartitionItem<Ny> *py, const char *oy,
                     const Coor<Ny> &fromy, const Coor<Ny> &sizey, const Coor<Ny> &dimy,
                     char okr, T **vy, const Context *ctx, sbx_comm comm, CoorOrder co,
                     Request *request, Session session, bool just_local = false) {
    check_session(session);
    const auto a = scalar(alpha), b = scalar(beta);
    const auto c = contexts(ctx, ncomponents);
    sbx_request h = nullptr;
    check(sbx_bsr_krylov_req(reinterpret_cast<sbx_bsr>(bsrh), (int)Nd, (int)Ni, (int)Nx, (int)Ny,
                             dtype<T>::value, a.data(), oim, odm, parts(px), ncomponents, ox,
                             fromx.data(), sizex.data(), dimx.data(), (const void *const *)vx,
                             b.data(), parts(py), oy, fromy.data(), sizey.data(), dimy.data(),
                             okr, (void *const *)vy, c.data(), comm, co_of(co), 0,
                             just_local ? 1 : 0, request ? &h : nullptr));
    if (request) *request = request_of(h);
}

} // namespace sbx_detail

// ---- runtime (platform.h:818-838, blas.h:965-974, alloc.h:398-443, performance.h:356-518) ----

inline unsigned int getGpuDevicesCount() {
    int n = 0;
    sbx_detail::check(sbx_get_gpu_devices_count(&n));
    return (unsigned int)n;
}
inline void clearHandles() { sbx_detail::check(sbx_clear_handles()); }
inline void clearCaches() { sbx_detail::check(sbx_clear_caches()); }
inline void sync(Context ctx) {
    sbx_context c = sbx_detail::contexts(&ctx, 1)[0];
    sbx_detail::check(sbx_sync(c));
}
template <typename T> T *allocate(std::size_t n, Context ctx) {
    void *p = nullptr;
    sbx_context c = sbx_detail::contexts(&ctx, 1)[0];
    sbx_detail::check(sbx_allocate((unsigned long long)(n * sizeof(T)), c, &p));
    return (T *)p;
}
template <typename T> void deallocate(T *ptr, Context ctx) {
    sbx_context c = sbx_detail::contexts(&ctx, 1)[0];
    sbx_detail::check(sbx_deallocate((void *)ptr, c));
}
/// Custom allocator hooks (platform.h:117-139): assign a function to the returned reference and
/// the library takes its device memory from it (return nullptr to fall back to hipMalloc)
using Allocator = std::function<void *(std::size_t, enum platform)>;
using Deallocator = std::function<void(void *, enum platform)>;
namespace sbx_detail {
inline Allocator &allocator_storage() {
    static Allocator a{};
    return a;
}
inline Deallocator &deallocator_storage() {
    static Deallocator d{};
    return d;
}
inline void *alloc_trampoline(unsigned long long bytes, int device, void *) {
    Allocator &a = allocator_storage();
    if (!a) return nullptr;
    (void)device; // the library makes `device` current before calling
    return a((std::size_t)bytes, GPU);
}
inline void free_trampoline(void *p, int, void *) {
    Deallocator &d = deallocator_storage();
    if (d) d(p, GPU);
}
inline void install_allocator_hooks() {
    static bool done = false;
    if (done) return;
    done = true;
    check(sbx_set_custom_allocator(alloc_trampoline, free_trampoline, nullptr));
}
} // namespace sbx_detail
inline Allocator &getCustomAllocator() {
    sbx_detail::install_allocator_hooks();
    return sbx_detail::allocator_storage();
}
inline Deallocator &getCustomDeallocator() {
    sbx_detail::install_allocator_hooks();
    return sbx_detail::deallocator_storage();
}

/// A buffer of the library's scratch cache (alloc.h:428-435); returned to the cache on release
template <typename T> std::shared_ptr<char> allocate_from_cache(std::size_t n, Context ctx) {
    sbx_context c = sbx_detail::contexts(&ctx, 1)[0];
    void *p = nullptr;
    sbx_detail::check(sbx_allocate_from_cache((unsigned long long)(n * sizeof(T)), c, &p));
    return std::shared_ptr<char>((char *)p, [c](char *q) { (void)sbx_release_to_cache(q, c); });
}

/// Scratch-cache usage per device (performance.h:436-495)
template <typename OStream> void reportCacheUsage(OStream &s) {
    const unsigned int n = getGpuDevicesCount();
    for (unsigned int d = 0; d < n; ++d) {
        unsigned long long cached = 0, live = 0;
        sbx_detail::check(sbx_cache_usage((int)d, &cached, &live));
        s << "superbblas_amd cache on GPU " << d << ": " << cached / 1048576.0 << " MiB idle, "
          << live / 1048576.0 << " MiB in use" << std::endl;
    }
}
/// Report scratch buffers still in use (performance.h:497-518)
template <typename OStream> void checkForMemoryLeaks(OStream &s) {
    const unsigned int n = getGpuDevicesCount();
    for (unsigned int d = 0; d < n; ++d) {
        unsigned long long cached = 0, live = 0;
        sbx_detail::check(sbx_cache_usage((int)d, &cached, &live));
        if (live) s << "superbblas_amd: " << live << " bytes of scratch still in use on GPU " << d
                    << std::endl;
    }
}

/// Kernel timings (HIP events per kernel family, performance.h:356-434): recorded while
/// getTrackingTime() (SB_TRACK_TIME=1) is on; reportTimings prints nothing otherwise
inline void resetTimings() {
    sbx_detail::sync_tracking();
    sbx_detail::check(sbx_timings_reset());
}
template <typename OStream> void reportTimings(OStream &s) {
    sbx_detail::sync_tracking();
    if (!getTrackingTime()) return;
    std::vector<char> buf(1 << 16);
    sbx_detail::check(sbx_timings_report(buf.data(), (int)buf.size()));
    s << "superbblas_amd kernel timings (family calls total_ms)\n" << buf.data();
}

// ---- partitioning helpers (dist.h:3318-3509, 3802-3825) ----

template <std::size_t Nd>
Coor<Nd> partitioning_distributed_procs(const char *order, const Coor<Nd> &dim,
                                        const char *dist_labels, unsigned int nprocs) {
    Coor<Nd> p{};
    sbx_detail::check(sbx_partitioning_distributed_procs((int)Nd, order, dim.data(), dist_labels,
                                                         (int)nprocs, p.data()));
    return p;
}

template <std::size_t Nd>
std::vector<PartitionItem<Nd>> basic_partitioning(const char *order, Coor<Nd> dim,
                                                  Coor<Nd> procs, const char *dist_labels,
                                                  int nprocs = -1, int ncomponents = 1) {
    long vp = 1;
    for (auto x : procs) vp *= x;
    const long nitems = (nprocs > vp ? nprocs : vp) * (long)(ncomponents > 0 ? ncomponents : 1);
    std::vector<PartitionItem<Nd>> r(nitems);
    sbx_detail::check(sbx_basic_partitioning((int)Nd, order, dim.data(), procs.data(),
                                             dist_labels, nprocs, ncomponents,
                                             reinterpret_cast<int *>(r.data())));
    return r;
}

template <std::size_t Nd>
std::vector<PartitionItem<Nd>> basic_partitioning(Coor<Nd> dim, Coor<Nd> procs, int nprocs = -1,
                                                  bool replicate = false,
                                                  Coor<Nd> ext_power = {{}}) {
    long vp = 1;
    for (auto x : procs) vp *= x;
    std::vector<PartitionItem<Nd>> r(nprocs > vp ? nprocs : vp);
    sbx_detail::check(sbx_basic_partitioning_ext((int)Nd, dim.data(), procs.data(), nprocs,
                                                 replicate ? 1 : 0, ext_power.data(),
                                                 reinterpret_cast<int *>(r.data())));
    return r;
}

template <std::size_t N>
std::vector<std::array<Coor<N>, 2>> make_hole(const Coor<N> &from, const Coor<N> &size,
                                              const Coor<N> &hole_from, const Coor<N> &hole_size,
                                              const Coor<N> &dim) {
    const int maxout = 4 * (int)(N > 0 ? N : 1) * (1 << (N < 6 ? N : 6));
    std::vector<std::array<Coor<N>, 2>> r(maxout);
    int nout = 0;
    sbx_detail::check(sbx_make_hole((int)N, from.data(), size.data(), hole_from.data(),
                                    hole_size.data(), dim.data(), maxout,
                                    reinterpret_cast<int *>(r.data()), &nout));
    r.resize(nout);
    return r;
}

// ---- copy (dist.h:3583-3602, 3534-3558) ----

template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void copy(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> from0, const Coor<Nd0> size0, const Coor<Nd0> dim0,
          const T **v0, const MaskType **mask0, const Context *ctx0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> from1, const Coor<Nd1> dim1, Q **v1,
          const MaskType **mask1, const Context *ctx1, CoorOrder co, CopyAdd copyadd,
          Request *request = nullptr, Session session = 0) {
    sbx_detail::copy_impl<Nd0, Nd1, T, Q>(alpha, p0, ncomponents0, o0, from0, size0, dim0, v0,
                                          mask0, ctx0, p1, ncomponents1, o1, from1, dim1, v1,
                                          mask1, ctx1, nullptr, co, copyadd, request, session);
}

template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void copy(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
          const T **v0, const MaskType **mask0, const Context *ctx0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1, Q **v1,
          const MaskType **mask1, const Context *ctx1, Communicator comm, CoorOrder co,
          CopyAdd copyadd, Request *request = nullptr, Session session = 0) {
    sbx_detail::copy_impl<Nd0, Nd1, T, Q>(alpha, p0, ncomponents0, o0, from0, size0, dim0, v0,
                                          mask0, ctx0, p1, ncomponents1, o1, from1, dim1, v1,
                                          mask1, ctx1, comm, co, copyadd, request, session);
}

// ---- contraction (dist.h:3701-3731, 3628-3662) ----

template <std::size_t Nd0, std::size_t Nd1, std::size_t Ndo, typename T>
void contraction(T alpha, const PartitionItem<Nd0> *p0, const Coor<Nd0> from0,
                 const Coor<Nd0> size0, const Coor<Nd0> &dim0, int ncomponents0, const char *o0,
                 bool conj0, const T **v0, const Context *ctx0, const PartitionItem<Nd1> *p1,
                 const Coor<Nd1> &from1, const Coor<Nd1> &size1, const Coor<Nd1> &dim1,
                 int ncomponents1, const char *o1, bool conj1, const T **v1, const Context *ctx1,
                 T beta, const PartitionItem<Ndo> *pr, const Coor<Ndo> &fromr,
                 const Coor<Ndo> &sizer, const Coor<Ndo> &dimr, int ncomponentsr, const char *o_r,
                 T **vr, const Context *ctxr, CoorOrder co, Request *request = nullptr,
                 Session session = 0) {
    sbx_detail::contraction_impl<Nd0, Nd1, Ndo, T>(
        alpha, p0, from0, size0, dim0, ncomponents0, o0, conj0, v0, ctx0, p1, from1, size1, dim1,
        ncomponents1, o1, conj1, v1, ctx1, beta, pr, fromr, sizer, dimr, ncomponentsr, o_r, vr,
        ctxr, nullptr, co, request, session);
}

template <std::size_t Nd0, std::size_t Nd1, std::size_t Ndo, typename T>
void contraction(T alpha, const PartitionItem<Nd0> *p0, const Coor<Nd0> &from0,
                 const Coor<Nd0> &size0, const Coor<Nd0> &dim0, int ncomponents0, const char *o0,
                 bool conj0, const T **v0, const Context *ctx0, const PartitionItem<Nd1> *p1,
                 const Coor<Nd1> &from1, const Coor<Nd1> &size1, const Coor<Nd1> &dim1,
                 int ncomponents1, const char *o1, bool conj1, const T **v1, const Context *ctx1,
                 T beta, const PartitionItem<Ndo> *pr, const Coor<Ndo> &fromr,
                 const Coor<Ndo> &sizer, const Coor<Ndo> &dimr, int ncomponentsr, const char *o_r,
                 T **vr, const Context *ctxr, Communicator comm, CoorOrder co,
                 Request *request = nullptr, Session session = 0) {
    sbx_detail::contraction_impl<Nd0, Nd1, Ndo, T>(
        alpha, p0, from0, size0, dim0, ncomponents0, o0, conj0, v0, ctx0, p1, from1, size1, dim1,
        ncomponents1, o1, conj1, v1, ctx1, beta, pr, fromr, sizer, dimr, ncomponentsr, o_r, vr,
        ctxr, comm, co, request, session);
}

// ---- BSR operator (bsr.h:2440-2580, 2286-2398) ----

/// Mixed precision (an extension; the reference's bsr_krylov is one T throughout): an operator
/// of create_bsr<Nd, Ni, float> or <Nd, Ni, std::complex<float>> may be contracted by
/// bsr_krylov<Nd, Ni, Nx, Ny, T> with T the double counterpart (double, std::complex<double>) on
/// the same handle.  Every value is converted to double exactly where it is read -- in place, in
/// the caller's array, no converted copy is kept -- and products, sums, alpha, beta and y are
/// double: the result is the product of the up-converted operator with x.  Every other pair of
/// types, and any type difference on an operator of create_kron_bsr, throws as before -- unless
/// sbx_tune_set("bsr.kron_mixed", 1) (default 0, read at each bsr_krylov call): then an operator
/// of create_kron_bsr<Nd, Ni, float> or <Nd, Ni, std::complex<float>> (colour values and spin
/// matrices both in that type) is contracted with T the double counterpart in the same way, A x
/// and A^H x, both arrays read in place and widened where they are read.
/// The same one step down: an operator of create_bsr<Nd, Ni, float16> or
/// <Nd, Ni, complex_float16> (IEEE binary16 values, above) is contracted by bsr_krylov with T =
/// float / std::complex<float>; the values are widened to float exactly where they are read, and
/// products, sums, alpha, beta and y are float.  binary16 holds magnitudes up to 65504 (smallest
/// subnormal 2^-24): scale the operator into range and pass the scale in alpha.  Half operators
/// with double vectors throw.  create_kron_bsr<Nd, Ni, float16> and <Nd, Ni, complex_float16>
/// (colour values and spin matrices both in that type) throw "unsupported type" whatever
/// bsr.kron_mixed -- unless sbx_tune_set("bsr.kron_half", 1) (default 0): then the operator is
/// created and, with the key still at 1 at the bsr_krylov call, contracted with T = float /
/// std::complex<float>, A x and A^H x, both arrays read in place and widened where they are read.
///
/// The image side (x with the image labels, y = alpha A^H x) of a create_bsr operator: by default
/// the first such product makes a conjugated, regrouped copy of the value blocks that all later
/// A^H products read -- a snapshot (values changed in place afterwards show in A x, not in A^H x)
/// and as many device bytes again as the values.  sbx_tune_set("bsr.adj_inplace", 1) makes A^H
/// products read the caller's value array in place, as A does: no copy, and A^H follows the
/// changes (3x3 and 12x12 operators then give up their LDS-DMA kernels
/// on that side).  Operators of create_kron_bsr are always in place.
template <std::size_t Nd, std::size_t Ni, typename T>
void create_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi, const PartitionItem<Nd> *pdm,
                const Coor<Nd> &dimd, int ncomponents, const Coor<Ni> &blockim,
                const Coor<Nd> &blockdm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                const T **v, const Context *ctx, CoorOrder co, BSR_handle **bsrh,
                Session session = 0) {
    sbx_detail::create_bsr_impl<Nd, Ni, T>(pim, dimi, pdm, dimd, ncomponents, blockim, blockdm,
                                           blockImFast, ii, jj, v, ctx, nullptr, co, bsrh,
                                           session);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi, const PartitionItem<Nd> *pdm,
                const Coor<Nd> &dimd, int ncomponents, const Coor<Ni> &blockim,
                const Coor<Nd> &blockdm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                const T **v, const Context *ctx, Communicator comm, CoorOrder co,
                BSR_handle **bsrh, Session session = 0) {
    sbx_detail::create_bsr_impl<Nd, Ni, T>(pim, dimi, pdm, dimd, ncomponents, blockim, blockdm,
                                           blockImFast, ii, jj, v, ctx, comm, co, bsrh, session);
}

/// create_kron_bsr (bsr.h:2476-2490): kronv[c] holds one volume(kronim) x volume(krondm) matrix
/// per nonzero position of a block row; keep ii, jj, v and kronv allocated until destroy_bsr.
/// bsr_krylov contracts such an operator with either side: x with the domain labels gives A x,
/// x with the image labels A^H x (the reference's local Kronecker operators throw "unsupported
/// conjugation" for the latter, bsr.h:399, 1032); A^H reads v and kronv in place
template <std::size_t Nd, std::size_t Ni, typename T>
void create_kron_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi,
                     const PartitionItem<Nd> *pdm, const Coor<Nd> &dimd, int ncomponents,
                     const Coor<Ni> &blockim, const Coor<Nd> &blockdm, const Coor<Ni> &kronim,
                     const Coor<Nd> &krondm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                     const T **v, const T **kronv, const Context *ctx, CoorOrder co,
                     BSR_handle **bsrh, Session session = 0) {
    sbx_detail::create_kron_bsr_impl<Nd, Ni, T>(pim, dimi, pdm, dimd, ncomponents, blockim,
                                                blockdm, kronim, krondm, blockImFast, ii, jj, v,
                                                kronv, ctx, nullptr, co, bsrh, session);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_kron_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi,
                     const PartitionItem<Nd> *pdm, const Coor<Nd> &dimd, int ncomponents,
                     const Coor<Ni> &blockim, const Coor<Nd> &blockdm, const Coor<Ni> &kronim,
                     const Coor<Nd> &krondm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                     const T **v, const T **kronv, const Context *ctx, Communicator comm,
                     CoorOrder co, BSR_handle **bsrh, Session session = 0) {
    sbx_detail::create_kron_bsr_impl<Nd, Ni, T>(pim, dimi, pdm, dimd, ncomponents, blockim,
                                                blockdm, kronim, krondm, blockImFast, ii, jj, v,
                                                kronv, ctx, comm, co, bsrh, session);
}

inline void destroy_bsr(BSR_handle *bsrh) {
    sbx_detail::check(sbx_destroy_bsr(reinterpret_cast<sbx_bsr>(bsrh)));
}

template <std::size_t Nd, std::size_t Ni, std::size_t Nx, std::size_t Ny, typename T>
void bsr_krylov(T alpha, BSR_handle *bsrh, const char *oim, const char *odm,
                const PartitionItem<Nx> *px, int ncomponents, const char *ox,
                const Coor<Nx> &fromx, const Coor<Nx> &sizex, const Coor<Nx> &dimx, const T **vx,
                T beta, const PartitionItem<Ny> *py, const char *oy, const Coor<Ny> &fromy,
                const Coor<Ny> &sizey, const Coor<Ny> &dimy, char okr, T **vy,
                const Context *ctx, CoorOrder co, Request *request = nullptr,
                Session session = 0) {
    sbx_detail::bsr_krylov_impl<Nd, Ni, Nx, Ny, T>(alpha, bsrh, oim, odm, px, ncomponents, ox,
                                                   fromx, sizex, dimx, vx, beta, py, oy, fromy,
                                                   sizey, dimy, okr, vy, ctx, nullptr, co,
                                                   request, session);
}

template <std::size_t Nd, std::size_t Ni, std::size_t Nx, std::size_t Ny, typename T>
void bsr_krylov(T alpha, BSR_handle *bsrh, const char *oim, const char *odm,
                const PartitionItem<Nx> *px, int ncomponents, const char *ox,
                const Coor<Nx> &fromx, const Coor<Nx> &sizex, const Coor<Nx> &dimx, const T **vx,
                T beta, const PartitionItem<Ny> *py, const char *oy, const Coor<Ny> &fromy,
                const Coor<Ny> &sizey, const Coor<Ny> &dimy, char okr, T **vy,
                const Context *ctx, Communicator comm, CoorOrder co, Request *request = nullptr,
                bool just_local = false, Session session = 0) {
    sbx_detail::bsr_krylov_impl<Nd, Ni, Nx, Ny, T>(alpha, bsrh, oim, odm, px, ncomponents, ox,
                                                   fromx, sizex, dimx, vx, beta, py, oy, fromy,
                                                   sizey, dimy, okr, vy, ctx, comm, co, request,
                                                   session, just_local);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void bsr_get_preferred_layout(BSR_handle *bsrh, int ncomponents, const Context *ctx,
                              CoorOrder co, MatrixLayout *preferred_layout_for_x,
                              MatrixLayout *preferred_layout_for_y) {
    const auto c = sbx_detail::contexts(ctx, ncomponents);
    std::vector<int> lx(ncomponents), ly(ncomponents);
    sbx_detail::check(sbx_bsr_get_preferred_layout(reinterpret_cast<sbx_bsr>(bsrh), ncomponents,
                                                   c.data(), nullptr, sbx_detail::co_of(co),
                                                   lx.data(), ly.data()));
    for (int i = 0; i < ncomponents; ++i) {
        preferred_layout_for_x[i] = lx[i] == SBX_ROW_MAJOR ? RowMajor : ColumnMajor;
        preferred_layout_for_y[i] = ly[i] == SBX_ROW_MAJOR ? RowMajor : ColumnMajor;
    }
}

// ---- dense batched solvers (dense.h:1160-1290) ----

namespace sbx_detail {
template <std::size_t N, typename T, typename F>
void inplace_dense_impl(F fn, const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents,
                        const char *o, T **v, const char *orows, const char *ocols,
                        const Context *ctx, sbx_comm comm, CoorOrder co, Session session) {
    check_session(session);
    const auto c = contexts(ctx, ncomponents);
    check(fn((int)N, dtype<T>::value, parts(p), dim.data(), ncomponents, o, (void *const *)v,
             orows, ocols, c.data(), comm, co_of(co), 0));
}

template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T, typename F>
void solve_dense_impl(F fn, T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc,
                      int ncomponentsc, const char *oc, const T **vc, const char *orows,
                      const char *ocols, const Context *ctxc, const PartitionItem<Nx> *px,
                      const Coor<Nx> &dimx, int ncomponentsx, const char *ox, const T **vx,
                      const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
                      int ncomponentsy, const char *oy, T **vy, const Context *ctxy, sbx_comm comm,
                      CoorOrder co, Session session) {
    check_session(session);
    const auto a = scalar(alpha);
    const auto c0 = contexts(ctxc, ncomponentsc), c1 = contexts(ctxx, ncomponentsx),
               c2 = contexts(ctxy, ncomponentsy);
    check(fn((int)Nc, (int)Nx, (int)Ny, dtype<T>::value, a.data(), parts(pc), dimc.data(),
             ncomponentsc, oc, (const void *const *)vc, orows, ocols, c0.data(), parts(px),
             dimx.data(), ncomponentsx, ox, (const void *const *)vx, c1.data(), parts(py),
             dimy.data(), ncomponentsy, oy, (void *const *)vy, c2.data(), comm, co_of(co), 0));
}
} // namespace sbx_detail

/// cholesky: every matrix (rows orows x columns ocols, batch = the other labels) <- its upper
/// Cholesky factor U (A = U^H U), dense.h:1160-1175
template <std::size_t N, typename T>
void cholesky(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
              T **v, const char *orows, const char *ocols, const Context *ctx, CoorOrder co,
              Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_cholesky, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, nullptr, co, session);
}
template <std::size_t N, typename T>
void cholesky(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
              T **v, const char *orows, const char *ocols, const Context *ctx, Communicator comm,
              CoorOrder co, Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_cholesky, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, comm, co, session);
}

/// inversion: every matrix <- its inverse, dense.h:1274-1287
template <std::size_t N, typename T>
void inversion(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
               T **v, const char *orows, const char *ocols, const Context *ctx, CoorOrder co,
               Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_inversion, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, nullptr, co, session);
}
template <std::size_t N, typename T>
void inversion(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
               T **v, const char *orows, const char *ocols, const Context *ctx,
               Communicator comm, CoorOrder co, Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_inversion, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, comm, co, session);
}

/// trsm: y = alpha C^-1 x or alpha x C^-1 with C upper triangular, dense.h:1195-1222
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void trsm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, CoorOrder co,
          Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(sbx_trsm, alpha, pc, dimc, ncomponentsc, oc, vc,
                                                orows, ocols, ctxc, px, dimx, ncomponentsx, ox,
                                                vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
                                                nullptr, co, session);
}
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void trsm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, Communicator comm,
          CoorOrder co, Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(sbx_trsm, alpha, pc, dimc, ncomponentsc, oc, vc,
                                                orows, ocols, ctxc, px, dimx, ncomponentsx, ox,
                                                vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
                                                comm, co, session);
}

/// gesm: y = alpha C^-1 x for general C, dense.h:1239-1266
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void gesm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, CoorOrder co,
          Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(sbx_gesm, alpha, pc, dimc, ncomponentsc, oc, vc,
                                                orows, ocols, ctxc, px, dimx, ncomponentsx, ox,
                                                vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
                                                nullptr, co, session);
}
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void gesm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, Communicator comm,
          CoorOrder co, Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(sbx_gesm, alpha, pc, dimc, ncomponentsc, oc, vc,
                                                orows, ocols, ctxc, px, dimx, ncomponentsx, ox,
                                                vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
                                                comm, co, session);
}

// ---- tensor storage, the S3T file format (storage.h:2374-2617) ----

/// Type of the values (storage.h:63) and of checksum (storage.h:66-70)
enum values_datatype { FLOAT = 0, DOUBLE = 1, CFLOAT = 2, CDOUBLE = 3, CHAR = 4, INT = 5 };
enum checksum_type { NoChecksum = 0, GlobalChecksum = 1, BlockChecksum = 2 };

/// Handle to a tensor storage (storage.h:2127)
using Storage_handle = sbx_storage;

namespace detail {
/// The values type of a scalar type (storage.h:80-90)
template <typename T> values_datatype get_values_datatype();
template <> inline values_datatype get_values_datatype<float>() { return FLOAT; }
template <> inline values_datatype get_values_datatype<double>() { return DOUBLE; }
template <> inline values_datatype get_values_datatype<std::complex<float>>() { return CFLOAT; }
template <> inline values_datatype get_values_datatype<std::complex<double>>() { return CDOUBLE; }
template <> inline values_datatype get_values_datatype<int>() { return INT; }
template <> inline values_datatype get_values_datatype<char>() { return CHAR; }

/// Checksum value type and default block size (storage.h:689-693)
using checksum_t = std::uint32_t;
const std::size_t default_checksum_blocksize = 64 * 1024 * 1024; // 64 MiB

/// do_checksum (storage.h:701-731): CRC-32 of size elements of str continuing from
/// prev_checksum, or with checksum_blocksize > 0 the CRC of the CRCs of blocks of that many bytes
template <typename T>
checksum_t do_checksum(const T *str, std::size_t size = 1, std::size_t checksum_blocksize = 0,
                       checksum_t prev_checksum = 0) {
    unsigned out = 0;
    sbx_detail::check(sbx_checksum((const void *)str, (unsigned long long)(size * sizeof(T)),
                                   (unsigned long long)checksum_blocksize, prev_checksum, &out));
    return out;
}
} // namespace detail

namespace sbx_detail {
/// get_storage_context (storage.h:1630-1645): the template parameters must match the file
template <std::size_t Nd, typename T> inline sbx_storage storage_of(Storage_handle stoh) {
    int nd = 0, t = 0;
    check(sbx_storage_info(stoh, &nd, &t));
    if (t != dtype<T>::value)
        throw std::runtime_error(
            "The template parameter T does not match with the datatype of the storage");
    if (nd != (int)Nd)
        throw std::runtime_error("The template parameter Nd does not match with the number of "
                                 "dimensions of the storage");
    return stoh;
}
template <typename T> inline int storage_dtype() {
    static_assert(!std::is_same<T, std::size_t>::value, "storage: unsupported type");
    return dtype<T>::value;
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void save_impl(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
               const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0,
               const Coor<Nd0> &dim0, const T **v0, const Context *ctx0, const char *o1,
               const Coor<Nd1> &from1, Storage_handle stoh, sbx_comm comm, CoorOrder co,
               Session session) {
    check_session(session);
    const auto a = scalar(alpha);
    const auto c = contexts(ctx0, ncomponents0);
    check(sbx_storage_save((int)Nd0, (int)Nd1, a.data(), dtype<T>::value, parts(p0),
                           ncomponents0, o0, from0.data(), size0.data(), dim0.data(),
                           (const void *const *)v0, c.data(), o1, from1.data(),
                           storage_of<Nd1, Q>(stoh), comm, co_of(co), 0));
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void load_impl(typename elem<T>::type alpha, Storage_handle stoh, const char *o0,
               const Coor<Nd0> &from0, const Coor<Nd0> &size0, const PartitionItem<Nd1> *p1,
               int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1,
               Q **v1, const Context *ctx1, sbx_comm comm, CoorOrder co, CopyAdd copyadd,
               Session session) {
    check_session(session);
    const auto a = scalar(alpha);
    const auto c = contexts(ctx1, ncomponents1);
    check(sbx_storage_load((int)Nd0, (int)Nd1, a.data(), storage_of<Nd0, T>(stoh), o0,
                           from0.data(), size0.data(), dtype<Q>::value, parts(p1), ncomponents1,
                           o1, from1.data(), dim1.data(), (void *const *)v1, c.data(), comm,
                           co_of(co), copyadd == Add ? SBX_ADD : SBX_COPY, 0));
}
template <std::size_t Nd0, std::size_t Nd1, typename Q>
void append_impl(const PartitionItem<Nd0> *p0, int num_blocks, const char *o0,
                 const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
                 const char *o1, const Coor<Nd1> &from1, Storage_handle stoh, sbx_comm comm,
                 CoorOrder co) {
    check(sbx_storage_append_blocks((int)Nd0, (int)Nd1, parts(p0), num_blocks, o0, from0.data(),
                                    size0.data(), dim0.data(), o1, from1.data(),
                                    storage_of<Nd1, Q>(stoh), comm, co_of(co)));
}
template <std::size_t N> inline std::string trivial_order() {
    std::string o(N, 'a');
    for (std::size_t i = 0; i < N; ++i) o[i] = (char)('a' + i);
    return o;
}
inline void read_header_impl(const char *filename, CoorOrder co, values_datatype &values_dtype,
                             std::vector<char> &metadata, std::vector<IndexType> &size) {
    int t = 0, ml = 0, nd = 0;
    check(sbx_storage_read_header(filename, co_of(co), &t, nullptr, 0, &ml, &nd, nullptr, 0));
    metadata.resize(ml);
    size.resize(nd);
    check(sbx_storage_read_header(filename, co_of(co), &t, metadata.data(), ml, &ml, &nd,
                                  size.data(), nd));
    switch (t) {
    case SBX_FLOAT: values_dtype = FLOAT; break;
    case SBX_DOUBLE: values_dtype = DOUBLE; break;
    case SBX_CFLOAT: values_dtype = CFLOAT; break;
    case SBX_CDOUBLE: values_dtype = CDOUBLE; break;
    default: values_dtype = INT; break;
    }
}
} // namespace sbx_detail

/// create_storage: a new file for a tensor of dims `dim` (its content, if any, is lost),
/// storage.h:2386-2395
template <std::size_t Nd, typename T>
void create_storage(const Coor<Nd> &dim, CoorOrder co, const char *filename,
                    const char *metadata, int metadata_length, checksum_type checksum,
                    Storage_handle *stoh) {
    sbx_detail::check(sbx_storage_create((int)Nd, dim.data(), sbx_detail::co_of(co), filename,
                                         metadata, metadata_length, (int)checksum,
                                         sbx_detail::storage_dtype<T>(), nullptr, stoh));
}
template <std::size_t Nd, typename T>
void create_storage(const Coor<Nd> &dim, CoorOrder co, const char *filename,
                    const char *metadata, int metadata_length, checksum_type checksum,
                    Communicator comm, Storage_handle *stoh) {
    sbx_detail::check(sbx_storage_create((int)Nd, dim.data(), sbx_detail::co_of(co), filename,
                                         metadata, metadata_length, (int)checksum,
                                         sbx_detail::storage_dtype<T>(), comm, stoh));
}

/// read_storage_header: values type, metadata and dims of a file, storage.h:2405-2421
inline void read_storage_header(const char *filename, CoorOrder co,
                                values_datatype &values_dtype, std::vector<char> &metadata,
                                std::vector<IndexType> &size) {
    sbx_detail::read_header_impl(filename, co, values_dtype, metadata, size);
}

/// open_storage: open an existing file, storage.h:2469-2476
template <std::size_t Nd, typename T>
void open_storage(const char *filename, bool allow_writing, Storage_handle *stoh) {
    sbx_detail::check(sbx_storage_open((int)Nd, sbx_detail::storage_dtype<T>(), filename,
                                       allow_writing ? 1 : 0, nullptr, stoh));
}
template <std::size_t Nd, typename T>
void open_storage(const char *filename, bool allow_writing, Communicator comm,
                  Storage_handle *stoh) {
    sbx_detail::check(sbx_storage_open((int)Nd, sbx_detail::storage_dtype<T>(), filename,
                                       allow_writing ? 1 : 0, comm, stoh));
}

/// append_blocks: declare blocks as stored (in the storage's coordinates), storage.h:2484-2495
template <std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd1> *p, int num_blocks, const Coor<Nd1> &dim,
                   Storage_handle stoh, CoorOrder co) {
    const std::string o = sbx_detail::trivial_order<Nd1>();
    sbx_detail::append_impl<Nd1, Nd1, Q>(p, num_blocks, o.c_str(), Coor<Nd1>{{}}, dim, dim,
                                         o.c_str(), Coor<Nd1>{{}}, stoh, nullptr, co);
}
template <std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd1> *p, int num_blocks, const Coor<Nd1> &dim,
                   Storage_handle stoh, Communicator comm, CoorOrder co) {
    const std::string o = sbx_detail::trivial_order<Nd1>();
    sbx_detail::append_impl<Nd1, Nd1, Q>(p, num_blocks, o.c_str(), Coor<Nd1>{{}}, dim, dim,
                                         o.c_str(), Coor<Nd1>{{}}, stoh, comm, co);
}
/// append_blocks: blocks of a tensor (labels o0) restricted to [from0, from0+size0) and placed
/// at from1 on the storage (labels o1), storage.h:2509-2521
template <std::size_t Nd0, std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd0> *p0, int num_blocks, const char *o0,
                   const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> dim0,
                   const char *o1, const Coor<Nd1> &from1, Storage_handle stoh, CoorOrder co) {
    sbx_detail::append_impl<Nd0, Nd1, Q>(p0, num_blocks, o0, from0, size0, dim0, o1, from1, stoh,
                                         nullptr, co);
}
template <std::size_t Nd0, std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd0> *p0, int num_blocks, const char *o0,
                   const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> dim0,
                   const char *o1, const Coor<Nd1> &from1, Storage_handle stoh,
                   Communicator comm, CoorOrder co) {
    sbx_detail::append_impl<Nd0, Nd1, Q>(p0, num_blocks, o0, from0, size0, dim0, o1, from1, stoh,
                                         comm, co);
}

/// save: alpha * v0[from0:from0+size0] into the stored blocks at from1, storage.h:2539-2554
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void save(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
          const T **v0, const Context *ctx0, const char *o1, const Coor<Nd1> &from1,
          Storage_handle stoh, CoorOrder co, Session session = 0) {
    sbx_detail::save_impl<Nd0, Nd1, T, Q>(alpha, p0, ncomponents0, o0, from0, size0, dim0, v0,
                                          ctx0, o1, from1, stoh, nullptr, co, session);
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void save(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
          const T **v0, const Context *ctx0, const char *o1, const Coor<Nd1> &from1,
          Storage_handle stoh, Communicator comm, CoorOrder co, Session session = 0) {
    sbx_detail::save_impl<Nd0, Nd1, T, Q>(alpha, p0, ncomponents0, o0, from0, size0, dim0, v0,
                                          ctx0, o1, from1, stoh, comm, co, session);
}

/// load: v1[from1 + P(c - from0)] = alpha * sto[c] for the stored c in [from0, from0+size0)
/// (Add copies as well, as the reference's local_load does), storage.h:2571-2595
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void load(typename elem<T>::type alpha, Storage_handle stoh, const char *o0,
          const Coor<Nd0> from0, const Coor<Nd0> size0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1,
          Q **v1, const Context *ctx1, CoorOrder co, CopyAdd copyadd, Session session = 0) {
    sbx_detail::load_impl<Nd0, Nd1, T, Q>(alpha, stoh, o0, from0, size0, p1, ncomponents1, o1,
                                          from1, dim1, v1, ctx1, nullptr, co, copyadd, session);
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void load(typename elem<T>::type alpha, Storage_handle stoh, const char *o0,
          const Coor<Nd0> &from0, const Coor<Nd0> &size0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1,
          Q **v1, const Context *ctx1, Communicator comm, CoorOrder co, CopyAdd copyadd,
          Session session = 0) {
    sbx_detail::load_impl<Nd0, Nd1, T, Q>(alpha, stoh, o0, from0, size0, p1, ncomponents1, o1,
                                          from1, dim1, v1, ctx1, comm, co, copyadd, session);
}

/// get_blocks: stored boxes overlapping [from1, from1+size1) of a tensor with labels o1,
/// relative to from1, storage.h:2608-2617
template <std::size_t Nd0, std::size_t Nd1, typename T>
void get_blocks(Storage_handle stoh, const char *o0, const char *o1, const Coor<Nd1> from1,
                const Coor<Nd1> size1, std::vector<PartitionItem<Nd1>> &blocks, CoorOrder co) {
    sbx_storage s = sbx_detail::storage_of<Nd0, T>(stoh);
    int n = 0;
    sbx_detail::check(sbx_storage_get_blocks(s, (int)Nd0, (int)Nd1, o0, o1, from1.data(),
                                             size1.data(), sbx_detail::co_of(co), nullptr, 0,
                                             &n));
    const std::size_t first = blocks.size();
    blocks.resize(first + n);
    sbx_detail::check(sbx_storage_get_blocks(
        s, (int)Nd0, (int)Nd1, o0, o1, from1.data(), size1.data(), sbx_detail::co_of(co),
        reinterpret_cast<int *>(blocks.data() + first), n, &n));
}

/// check_storage: verify the checksums, storage.h:2439-2446
template <std::size_t Nd1, typename Q> void check_storage(Storage_handle stoh) {
    sbx_detail::check(sbx_storage_check(sbx_detail::storage_of<Nd1, Q>(stoh), nullptr));
}
template <std::size_t Nd1, typename Q> void check_storage(Storage_handle stoh, Communicator comm) {
    sbx_detail::check(sbx_storage_check(sbx_detail::storage_of<Nd1, Q>(stoh), comm));
}

/// close_storage: write the pending checksums and release the handle, storage.h:2451-2460
template <std::size_t Nd1, typename Q> void close_storage(Storage_handle stoh) {
    sbx_detail::check(sbx_storage_close(sbx_detail::storage_of<Nd1, Q>(stoh), nullptr));
}
template <std::size_t Nd1, typename Q> void close_storage(Storage_handle stoh, Communicator comm) {
    sbx_detail::check(sbx_storage_close(sbx_detail::storage_of<Nd1, Q>(stoh), comm));
}

/// preallocate_storage / flush_storage, storage.h:2427-2434
inline void preallocate_storage(Storage_handle stoh, std::size_t size) {
    sbx_detail::check(sbx_storage_preallocate(stoh, (unsigned long long)size));
}
inline void flush_storage(Storage_handle stoh) { sbx_detail::check(sbx_storage_flush(stoh)); }

// ---- MPI overloads: RCCL (one GPU per rank) or host staging over MPI_Alltoallv ----
#ifdef SUPERBBLAS_USE_MPI
namespace sbx_detail {
inline int mpi_alltoallv(const void *sbuf, const unsigned long long *sbytes,
                         const unsigned long long *sdispl, void *rbuf,
                         const unsigned long long *rbytes, const unsigned long long *rdispl,
                         void *user) {
    MPI_Comm comm = *(MPI_Comm *)user;
    int n = 0;
    MPI_Comm_size(comm, &n);
    std::vector<int> sc(n), sd(n), rc(n), rd(n);
    for (int i = 0; i < n; ++i) {
        if (sbytes[i] > 0x7fffffffULL || sdispl[i] > 0x7fffffffULL || rbytes[i] > 0x7fffffffULL ||
            rdispl[i] > 0x7fffffffULL)
            return 1; // exchanges of 2 GiB or more per call need the RCCL transport
        sc[i] = (int)sbytes[i];
        sd[i] = (int)sdispl[i];
        rc[i] = (int)rbytes[i];
        rd[i] = (int)rdispl[i];
    }
    return MPI_Alltoallv(sbuf, sc.data(), sd.data(), MPI_BYTE, rbuf, rc.data(), rd.data(),
                         MPI_BYTE, comm) == MPI_SUCCESS
               ? 0
               : 1;
}
/// Whether every rank of `mpicomm` drives its own GPU: ranks on one node (MPI_COMM_TYPE_SHARED)
/// must hold distinct device ids (RCCL runs one rank per device, like the reference's GPU-aware
/// MPI path, dist.h:1626-1641)
inline bool ranks_own_devices(MPI_Comm mpicomm, int device) {
    MPI_Comm node;
    if (MPI_Comm_split_type(mpicomm, MPI_COMM_TYPE_SHARED, 0, MPI_INFO_NULL, &node) != MPI_SUCCESS)
        return false;
    int n = 1;
    MPI_Comm_size(node, &n);
    std::vector<int> devs(n);
    MPI_Allgather(&device, 1, MPI_INT, devs.data(), 1, MPI_INT, node);
    MPI_Comm_free(&node);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (devs[i] == devs[j]) return false;
    return true;
}

/// One communicator per MPI_Comm, created on first use (device = the first GPU context's
/// device) and kept for the life of the process.  Transport: RCCL over xGMI when every rank
/// drives its own GPU -- the unique id is made by rank 0 and broadcast with MPI_Bcast, so device
/// buffers travel directly (the reference's GPU-aware MPI path, dist.h:1626-1641, 1702-1773) --
/// otherwise (ranks sharing a GPU) the host-staged transport over MPI_Alltoallv
/// (dist.h:1426-1500).  SB_MPI_GPU (runtime_features.h:118-133) forces one: != 0 passes device
/// buffers to the transport (RCCL), 0 stages them through host memory;
/// SUPERBBLAS_AMD_MPI_TRANSPORT=host|rccl is an older spelling of the same choice.
inline sbx_comm comm_of(MPI_Comm mpicomm, const Context *ctx, int ncomponents) {
    struct Entry {
        std::unique_ptr<MPI_Comm> c;
        sbx_comm h;
    };
    static std::vector<Entry> cache;
    for (auto &e : cache) {
        int same = MPI_UNEQUAL;
        MPI_Comm_compare(*e.c, mpicomm, &same);
        if (same == MPI_IDENT) return e.h;
    }
    int rank = 0, n = 1, device = 0;
    MPI_Comm_rank(mpicomm, &rank);
    MPI_Comm_size(mpicomm, &n);
    for (int i = 0; i < ncomponents; ++i)
        if (ctx[i].plat != CPU) {
            device = ctx[i].device;
            break;
        }
    const char *force = std::getenv("SUPERBBLAS_AMD_MPI_TRANSPORT");
    bool rccl = ranks_own_devices(mpicomm, device); // collective: every rank decides alike
    if (force && std::string(force) == "host") rccl = false;
    if (force && std::string(force) == "rccl") rccl = true;
    if (getUseMPIGpu() != 0) rccl = getUseMPIGpu() > 0;
    Entry e{std::unique_ptr<MPI_Comm>(new MPI_Comm(mpicomm)), nullptr};
    if (rccl) {
        unsigned char id[128] = {0};
        if (rank == 0) check(sbx_comm_unique_id(id));
        MPI_Bcast(id, 128, MPI_BYTE, 0, mpicomm);
        check(sbx_comm_create(n, rank, id, device, &e.h));
    } else {
        check(sbx_comm_create_host(n, rank, device, mpi_alltoallv, e.c.get(), &e.h));
    }
    cache.push_back(std::move(e));
    return cache.back().h;
}
} // namespace sbx_detail

template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void copy(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
          const T **v0, const MaskType **mask0, const Context *ctx0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1, Q **v1,
          const MaskType **mask1, const Context *ctx1, MPI_Comm mpicomm, CoorOrder co,
          CopyAdd copyadd, Request *request = nullptr, Session session = 0) {
    sbx_detail::copy_impl<Nd0, Nd1, T, Q>(
        alpha, p0, ncomponents0, o0, from0, size0, dim0, v0, mask0, ctx0, p1, ncomponents1, o1,
        from1, dim1, v1, mask1, ctx1, sbx_detail::comm_of(mpicomm, ctx1, ncomponents1), co,
        copyadd, request, session);
}

template <std::size_t Nd0, std::size_t Nd1, std::size_t Ndo, typename T>
void contraction(T alpha, const PartitionItem<Nd0> *p0, const Coor<Nd0> &from0,
                 const Coor<Nd0> &size0, const Coor<Nd0> &dim0, int ncomponents0, const char *o0,
                 bool conj0, const T **v0, const Context *ctx0, const PartitionItem<Nd1> *p1,
                 const Coor<Nd1> &from1, const Coor<Nd1> &size1, const Coor<Nd1> &dim1,
                 int ncomponents1, const char *o1, bool conj1, const T **v1, const Context *ctx1,
                 T beta, const PartitionItem<Ndo> *pr, const Coor<Ndo> &fromr,
                 const Coor<Ndo> &sizer, const Coor<Ndo> &dimr, int ncomponentsr, const char *o_r,
                 T **vr, const Context *ctxr, MPI_Comm mpicomm, CoorOrder co,
                 Request *request = nullptr, Session session = 0) {
    sbx_detail::contraction_impl<Nd0, Nd1, Ndo, T>(
        alpha, p0, from0, size0, dim0, ncomponents0, o0, conj0, v0, ctx0, p1, from1, size1, dim1,
        ncomponents1, o1, conj1, v1, ctx1, beta, pr, fromr, sizer, dimr, ncomponentsr, o_r, vr,
        ctxr, sbx_detail::comm_of(mpicomm, ctxr, ncomponentsr), co, request, session);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi, const PartitionItem<Nd> *pdm,
                const Coor<Nd> &dimd, int ncomponents, const Coor<Ni> &blockim,
                const Coor<Nd> &blockdm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                const T **v, const Context *ctx, MPI_Comm mpicomm, CoorOrder co, BSR_handle **bsrh,
                Session session = 0) {
    sbx_detail::create_bsr_impl<Nd, Ni, T>(pim, dimi, pdm, dimd, ncomponents, blockim, blockdm,
                                           blockImFast, ii, jj, v, ctx,
                                           sbx_detail::comm_of(mpicomm, ctx, ncomponents), co,
                                           bsrh, session);
}

template <std::size_t Nd, std::size_t Ni, typename T>
void create_kron_bsr(const PartitionItem<Ni> *pim, const Coor<Ni> &dimi,
                     const PartitionItem<Nd> *pdm, const Coor<Nd> &dimd, int ncomponents,
                     const Coor<Ni> &blockim, const Coor<Nd> &blockdm, const Coor<Ni> &kronim,
                     const Coor<Nd> &krondm, bool blockImFast, IndexType **ii, Coor<Nd> **jj,
                     const T **v, const T **kronv, const Context *ctx, MPI_Comm mpicomm,
                     CoorOrder co, BSR_handle **bsrh, Session session = 0) {
    sbx_detail::create_kron_bsr_impl<Nd, Ni, T>(
        pim, dimi, pdm, dimd, ncomponents, blockim, blockdm, kronim, krondm, blockImFast, ii, jj,
        v, kronv, ctx, sbx_detail::comm_of(mpicomm, ctx, ncomponents), co, bsrh, session);
}

template <std::size_t Nd, std::size_t Ni, std::size_t Nx, std::size_t Ny, typename T>
void bsr_krylov(T alpha, BSR_handle *bsrh, const char *oim, const char *odm,
                const PartitionItem<Nx> *px, int ncomponents, const char *ox,
                const Coor<Nx> &fromx, const Coor<Nx> &sizex, const Coor<Nx> &dimx, const T **vx,
                T beta, const PartitionItem<Ny> *py, const char *oy, const Coor<Ny> &fromy,
                const Coor<Ny> &sizey, const Coor<Ny> &dimy, char okr, T **vy,
                const Context *ctx, MPI_Comm mpicomm, CoorOrder co, Request *request = nullptr,
                bool just_local = false, Session session = 0) {
    sbx_detail::bsr_krylov_impl<Nd, Ni, Nx, Ny, T>(
        alpha, bsrh, oim, odm, px, ncomponents, ox, fromx, sizex, dimx, vx, beta, py, oy, fromy,
        sizey, dimy, okr, vy, ctx, sbx_detail::comm_of(mpicomm, ctx, ncomponents), co, request,
        session, just_local);
}
template <std::size_t Nd, std::size_t Ni, typename T>
void bsr_get_preferred_layout(BSR_handle *bsrh, int ncomponents, const Context *ctx,
                              MPI_Comm mpicomm, CoorOrder co,
                              MatrixLayout *preferred_layout_for_x,
                              MatrixLayout *preferred_layout_for_y) {
    const auto c = sbx_detail::contexts(ctx, ncomponents);
    std::vector<int> lx(ncomponents), ly(ncomponents);
    sbx_detail::check(sbx_bsr_get_preferred_layout(
        reinterpret_cast<sbx_bsr>(bsrh), ncomponents, c.data(),
        sbx_detail::comm_of(mpicomm, ctx, ncomponents), sbx_detail::co_of(co), lx.data(),
        ly.data()));
    for (int i = 0; i < ncomponents; ++i) {
        preferred_layout_for_x[i] = lx[i] == SBX_ROW_MAJOR ? RowMajor : ColumnMajor;
        preferred_layout_for_y[i] = ly[i] == SBX_ROW_MAJOR ? RowMajor : ColumnMajor;
    }
}

template <std::size_t N, typename T>
void cholesky(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
              T **v, const char *orows, const char *ocols, const Context *ctx, MPI_Comm mpicomm,
              CoorOrder co, Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_cholesky, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, sbx_detail::comm_of(mpicomm, ctx, ncomponents), co,
                                         session);
}
template <std::size_t N, typename T>
void inversion(const PartitionItem<N> *p, const Coor<N> &dim, int ncomponents, const char *o,
               T **v, const char *orows, const char *ocols, const Context *ctx, MPI_Comm mpicomm,
               CoorOrder co, Session session = 0) {
    sbx_detail::inplace_dense_impl<N, T>(sbx_inversion, p, dim, ncomponents, o, v, orows, ocols,
                                         ctx, sbx_detail::comm_of(mpicomm, ctx, ncomponents), co,
                                         session);
}
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void trsm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, MPI_Comm mpicomm,
          CoorOrder co, Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(
        sbx_trsm, alpha, pc, dimc, ncomponentsc, oc, vc, orows, ocols, ctxc, px, dimx,
        ncomponentsx, ox, vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
        sbx_detail::comm_of(mpicomm, ctxc, ncomponentsc), co, session);
}
template <std::size_t Nc, std::size_t Nx, std::size_t Ny, typename T>
void gesm(T alpha, const PartitionItem<Nc> *pc, const Coor<Nc> &dimc, int ncomponentsc,
          const char *oc, const T **vc, const char *orows, const char *ocols, const Context *ctxc,
          const PartitionItem<Nx> *px, const Coor<Nx> &dimx, int ncomponentsx, const char *ox,
          const T **vx, const Context *ctxx, const PartitionItem<Ny> *py, const Coor<Ny> &dimy,
          int ncomponentsy, const char *oy, T **vy, const Context *ctxy, MPI_Comm mpicomm,
          CoorOrder co, Session session = 0) {
    sbx_detail::solve_dense_impl<Nc, Nx, Ny, T>(
        sbx_gesm, alpha, pc, dimc, ncomponentsc, oc, vc, orows, ocols, ctxc, px, dimx,
        ncomponentsx, ox, vx, ctxx, py, dimy, ncomponentsy, oy, vy, ctxy,
        sbx_detail::comm_of(mpicomm, ctxc, ncomponentsc), co, session);
}
// storage over MPI (storage.h:2142-2370)
template <std::size_t Nd, typename T>
void create_storage(const Coor<Nd> &dim, CoorOrder co, const char *filename,
                    const char *metadata, int metadata_length, checksum_type checksum,
                    MPI_Comm mpicomm, Storage_handle *stoh) {
    create_storage<Nd, T>(dim, co, filename, metadata, metadata_length, checksum,
                          sbx_detail::comm_of(mpicomm, nullptr, 0), stoh);
}
inline void read_storage_header(const char *filename, CoorOrder co,
                                values_datatype &values_dtype, std::vector<char> &metadata,
                                std::vector<IndexType> &size, MPI_Comm) {
    sbx_detail::read_header_impl(filename, co, values_dtype, metadata, size);
}
template <std::size_t Nd, typename T>
void open_storage(const char *filename, bool allow_writing, MPI_Comm mpicomm,
                  Storage_handle *stoh) {
    open_storage<Nd, T>(filename, allow_writing, sbx_detail::comm_of(mpicomm, nullptr, 0), stoh);
}
template <std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd1> *p, int num_blocks, const Coor<Nd1> &dim,
                   Storage_handle stoh, MPI_Comm mpicomm, CoorOrder co) {
    append_blocks<Nd1, Q>(p, num_blocks, dim, stoh, sbx_detail::comm_of(mpicomm, nullptr, 0), co);
}
template <std::size_t Nd0, std::size_t Nd1, typename Q>
void append_blocks(const PartitionItem<Nd0> *p0, int num_blocks, const char *o0,
                   const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
                   const char *o1, const Coor<Nd1> &from1, Storage_handle stoh,
                   MPI_Comm mpicomm, CoorOrder co) {
    append_blocks<Nd0, Nd1, Q>(p0, num_blocks, o0, from0, size0, dim0, o1, from1, stoh,
                               sbx_detail::comm_of(mpicomm, nullptr, 0), co);
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void save(typename elem<T>::type alpha, const PartitionItem<Nd0> *p0, int ncomponents0,
          const char *o0, const Coor<Nd0> &from0, const Coor<Nd0> &size0, const Coor<Nd0> &dim0,
          const T **v0, const Context *ctx0, const char *o1, const Coor<Nd1> &from1,
          Storage_handle stoh, MPI_Comm mpicomm, CoorOrder co, Session session = 0) {
    sbx_detail::save_impl<Nd0, Nd1, T, Q>(alpha, p0, ncomponents0, o0, from0, size0, dim0, v0,
                                          ctx0, o1, from1, stoh,
                                          sbx_detail::comm_of(mpicomm, ctx0, ncomponents0), co,
                                          session);
}
template <std::size_t Nd0, std::size_t Nd1, typename T, typename Q>
void load(typename elem<T>::type alpha, Storage_handle stoh, const char *o0,
          const Coor<Nd0> &from0, const Coor<Nd0> &size0, const PartitionItem<Nd1> *p1,
          int ncomponents1, const char *o1, const Coor<Nd1> &from1, const Coor<Nd1> &dim1,
          Q **v1, const Context *ctx1, MPI_Comm mpicomm, CoorOrder co, CopyAdd copyadd,
          Session session = 0) {
    sbx_detail::load_impl<Nd0, Nd1, T, Q>(alpha, stoh, o0, from0, size0, p1, ncomponents1, o1,
                                          from1, dim1, v1, ctx1,
                                          sbx_detail::comm_of(mpicomm, ctx1, ncomponents1), co,
                                          copyadd, session);
}
template <std::size_t Nd0, std::size_t Nd1, typename T>
void get_blocks(Storage_handle stoh, const char *o0, const char *o1, const Coor<Nd1> from1,
                const Coor<Nd1> size1, std::vector<PartitionItem<Nd1>> &blocks, MPI_Comm,
                CoorOrder co) {
    get_blocks<Nd0, Nd1, T>(stoh, o0, o1, from1, size1, blocks, co);
}
template <std::size_t Nd1, typename Q> void check_storage(Storage_handle stoh, MPI_Comm mpicomm) {
    check_storage<Nd1, Q>(stoh, sbx_detail::comm_of(mpicomm, nullptr, 0));
}
template <std::size_t Nd1, typename Q> void close_storage(Storage_handle stoh, MPI_Comm mpicomm) {
    close_storage<Nd1, Q>(stoh, sbx_detail::comm_of(mpicomm, nullptr, 0));
}

#endif // SUPERBBLAS_USE_MPI

} // namespace superbblas

#include "superbblas_amd/detail.h"

#endif // SUPERBBLAS_AMD_SUPERBBLAS_H
