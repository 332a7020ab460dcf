// Half-precision operator values through the drop-in header (include/superbblas.h), compiled
// with plain g++ (no _Float16 needed): an operator of create_bsr<6, 6, complex_float16>
// contracted by bsr_krylov<6, 6, 8, 8, std::complex<float>> on the same handle, against a host
// loop in float on the widened values (integers of magnitude at most 6: their binary16 bit
// patterns come from a table, and every sum is exact); bsr_krylov<..., std::complex<double>> on
// that handle must throw std::runtime_error and leave y as it was.
#include "superbblas.h"

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

using namespace superbblas;
using Z = std::complex<double>;
using C = std::complex<float>;
using H = complex_float16;

static int failures = 0;
#define CHECK(c, msg)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            std::printf("FAIL: %s\n", msg);                                                        \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

// binary16 of an integer -6 .. 6: sign, exponent 15 + floor(log2 |i|), 10 mantissa bits
static float16 half_of(int i) {
    static const std::uint16_t mag[7] = {0x0000, 0x3C00, 0x4000, 0x4200, 0x4400, 0x4500, 0x4600};
    return float16{(std::uint16_t)(mag[i < 0 ? -i : i] | (i < 0 ? 0x8000 : 0))};
}
static int re_of(long g, int seed) { return (int)((7 * g + 3 + 13 * seed) % 11 - 5); }
static int im_of(long g, int seed) { return (int)((5 * g + 1 + 7 * seed) % 13 - 6); }

// host -> device and back as flat arrays through superbblas::copy
template <typename T> static T *upload(const std::vector<T> &h) {
    Context cpu = createCpuContext(), gpu = createGpuContext(0);
    T *d = allocate<T>(h.size(), gpu);
    const Coor<1> dn{(int)h.size()};
    PartitionItem<1> p{Coor<1>{}, dn};
    const T *src = h.data();
    copy<1, 1, T, T>(1, &p, 1, "i", Coor<1>{}, dn, dn, &src, nullptr, &cpu, &p, 1, "i", Coor<1>{}, dn,
                     &d, nullptr, &gpu, SlowToFast, Copy);
    return d;
}
template <typename T> static std::vector<T> download(const T *d, std::size_t n) {
    Context cpu = createCpuContext(), gpu = createGpuContext(0);
    std::vector<T> h(n);
    const Coor<1> dn{(int)n};
    PartitionItem<1> p{Coor<1>{}, dn};
    T *dst = h.data();
    copy<1, 1, T, T>(1, &p, 1, "i", Coor<1>{}, dn, dn, &d, nullptr, &gpu, &p, 1, "i", Coor<1>{}, dn,
                     &dst, nullptr, &cpu, SlowToFast, Copy);
    sync(gpu);
    return h;
}

int main() {
    if (getGpuDevicesCount() == 0) {
        std::printf("no GPU\n");
        return 2;
    }
    Context gpu = createGpuContext(0);
    // 2^4 lattice, 16x16 blocks (spin 2 x color 8), five per row: the site and its neighbour in
    // each direction
    const int L = 2, s = 2, c = 8, b = s * c, nb = 5, nc = 3;
    const Coor<6> dim{L, L, L, L, s, c};
    const long V = (long)L * L * L * L;
    std::vector<IndexType> ii(V, nb);
    std::vector<Coor<6>> jj;
    for (long i = 0; i < V; ++i) {
        Coor<6> cc{(int)(i / (L * L * L)), (int)(i / (L * L) % L), (int)(i / L % L), (int)(i % L), 0, 0};
        jj.push_back(cc);
        for (int d = 0; d < 4; ++d) {
            Coor<6> q = cc;
            q[d] = (q[d] + 1) % L;
            jj.push_back(q);
        }
    }
    // the values as complex_float16 and, widened, as complex<float>
    const long nv = V * nb * b * b;
    std::vector<H> hv(nv);
    std::vector<C> hvc(nv);
    for (long i = 0; i < nv; ++i) {
        hv[i] = H{half_of(re_of(i, 4)), half_of(im_of(i, 4))};
        hvc[i] = C((float)re_of(i, 4), (float)im_of(i, 4));
    }
    const Coor<8> dx{1, L, L, L, L, s, c, nc};
    const long nx = V * b * nc;
    std::vector<C> hx(nx), hy(nx, C(7));
    for (long i = 0; i < nx; ++i) hx[i] = C((float)re_of(i, 5), (float)im_of(i, 5));
    std::vector<Z> hxz(nx), hyz(nx, Z(7));
    for (long i = 0; i < nx; ++i) hxz[i] = Z(re_of(i, 5), im_of(i, 5));

    // the library copies no half tensors: the 4-byte values travel as the ints of their bits
    static_assert(sizeof(H) == sizeof(int), "a complex_float16 is one int of bits");
    std::vector<int> bits(nv);
    std::memcpy(bits.data(), hv.data(), nv * sizeof(int));
    const H *dv = (const H *)upload(bits);
    IndexType *dii = upload(ii);
    std::vector<IndexType> jflat((const IndexType *)jj.data(), (const IndexType *)jj.data() + jj.size() * 6);
    Coor<6> *djj = (Coor<6> *)upload(jflat);
    C *vx = upload(hx), *vy = upload(hy);
    Z *vxz = upload(hxz), *vyz = upload(hyz);

    PartitionItem<6> pop{Coor<6>{}, dim};
    PartitionItem<8> px{Coor<8>{}, dx};
    const Coor<6> block{1, 1, 1, 1, s, c};

    // complex_float16 operator, complex<float> vectors
    BSR_handle *op = nullptr;
    create_bsr<6, 6, H>(&pop, dim, &pop, dim, 1, block, block, false, &dii, &djj, &dv, &gpu, SlowToFast,
                        &op);
    const C *cx = vx;
    bsr_krylov<6, 6, 8, 8, C>(C(1), op, "xyztsc", "XYZTSC", &px, 1, "pXYZTSCn", {{}}, dx, dx, &cx, C(0),
                              &px, "pxyztscn", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    std::vector<C> out = download(vy, nx);
    bool ok = true;
    for (long r = 0; r < V; ++r)
        for (int i = 0; i < b; ++i)
            for (int col = 0; col < nc; ++col) {
                C acc = 0;
                for (int k = 0; k < nb; ++k) {
                    const Coor<6> &q = jj[r * nb + k];
                    const long site = ((q[0] * L + q[1]) * L + q[2]) * L + q[3];
                    for (int j = 0; j < b; ++j)
                        acc += hvc[((r * nb + k) * b + i) * b + j] * hx[(site * b + j) * nc + col];
                }
                ok &= out[(r * b + i) * nc + col] == acc;
            }
    CHECK(ok, "complex_float16 operator with complex<float> vectors");

    // double vectors on the same handle keep throwing and leave y as it was
    bool thrown = false;
    try {
        const Z *cxz = vxz;
        bsr_krylov<6, 6, 8, 8, Z>(Z(1), op, "xyztsc", "XYZTSC", &px, 1, "pXYZTSCn", {{}}, dx, dx, &cxz,
                                  Z(0), &px, "pxyztscn", {{}}, dx, dx, 'p', &vyz, &gpu, SlowToFast);
    } catch (const std::runtime_error &) { thrown = true; }
    CHECK(thrown, "complex_float16 operator with complex<double> vectors throws std::runtime_error");
    std::vector<Z> outz = download(vyz, nx);
    bool same = true;
    for (long i = 0; i < nx; ++i) same &= outz[i] == Z(7);
    CHECK(same, "a refused call leaves y untouched");
    destroy_bsr(op);

    deallocate((int *)dv, gpu);
    deallocate(dii, gpu);
    deallocate((IndexType *)djj, gpu);
    deallocate(vx, gpu);
    deallocate(vy, gpu);
    deallocate(vxz, gpu);
    deallocate(vyz, gpu);
    if (failures == 0) std::printf("half_bsr_test: all checks passed\n");
    return failures ? 1 : 0;
}
