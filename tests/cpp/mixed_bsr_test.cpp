// Mixed-precision bsr_krylov through the drop-in header (include/superbblas.h), compiled with
// plain g++: an operator of create_bsr<6, 6, std::complex<float>> contracted by
// bsr_krylov<6, 6, 8, 8, std::complex<double>> on the same handle, against a host loop in double
// on the up-converted values (integer-valued data: exact); the reverse pair (a complex<double>
// operator with complex<float> vectors) must throw std::runtime_error.
#include "superbblas.h"

#include <cstdio>
#include <stdexcept>
#include <vector>

using namespace superbblas;
using Z = std::complex<double>;
using C = std::complex<float>;

static int failures = 0;
#define CHECK(c, msg)                                                                              \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            std::printf("FAIL: %s\n", msg);                                                        \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

template <typename T> static T val(long g, int seed) {
    return T((typename T::value_type)((7 * g + 3 + 13 * seed) % 11 - 5),
             (typename T::value_type)((5 * g + 1 + 7 * seed) % 13 - 6));
}

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
    std::vector<C> hv(V * nb * b * b);
    for (long i = 0; i < (long)hv.size(); ++i) hv[i] = val<C>(i, 4);
    std::vector<Z> hvz(hv.size());
    for (long i = 0; i < (long)hv.size(); ++i) hvz[i] = Z(hv[i].real(), hv[i].imag());
    const Coor<8> dx{1, L, L, L, L, s, c, nc};
    const long nx = V * b * nc;
    std::vector<Z> hx(nx), hy(nx, Z(7));
    for (long i = 0; i < nx; ++i) hx[i] = val<Z>(i, 5);
    std::vector<C> hxc(nx), hyc(nx, C(7));
    for (long i = 0; i < nx; ++i) hxc[i] = val<C>(i, 5);

    C *dv = upload(hv);
    Z *dvz = upload(hvz);
    IndexType *dii = upload(ii);
    std::vector<IndexType> jflat((const IndexType *)jj.data(), (const IndexType *)jj.data() + jj.size() * 6);
    Coor<6> *djj = (Coor<6> *)upload(jflat);
    Z *vx = upload(hx), *vy = upload(hy);
    C *vxc = upload(hxc), *vyc = upload(hyc);

    PartitionItem<6> pop{Coor<6>{}, dim};
    PartitionItem<8> px{Coor<8>{}, dx};
    const Coor<6> block{1, 1, 1, 1, s, c};

    // complex<float> operator, complex<double> vectors
    BSR_handle *op = nullptr;
    const C *cv = dv;
    create_bsr<6, 6, C>(&pop, dim, &pop, dim, 1, block, block, false, &dii, &djj, &cv, &gpu, SlowToFast,
                        &op);
    const Z *cx = vx;
    bsr_krylov<6, 6, 8, 8, Z>(Z(1), op, "xyztsc", "XYZTSC", &px, 1, "pXYZTSCn", {{}}, dx, dx, &cx, Z(0),
                              &px, "pxyztscn", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    std::vector<Z> out = download(vy, nx);
    bool ok = true;
    for (long r = 0; r < V; ++r)
        for (int i = 0; i < b; ++i)
            for (int col = 0; col < nc; ++col) {
                Z acc = 0;
                for (int k = 0; k < nb; ++k) {
                    const Coor<6> &q = jj[r * nb + k];
                    const long site = ((q[0] * L + q[1]) * L + q[2]) * L + q[3];
                    for (int j = 0; j < b; ++j)
                        acc += hvz[((r * nb + k) * b + i) * b + j] * hx[(site * b + j) * nc + col];
                }
                ok &= out[(r * b + i) * nc + col] == acc;
            }
    CHECK(ok, "complex<float> operator with complex<double> vectors");
    destroy_bsr(op);

    // the reverse pair keeps throwing and leaves y as it was
    BSR_handle *opz = nullptr;
    const Z *cvz = dvz;
    create_bsr<6, 6, Z>(&pop, dim, &pop, dim, 1, block, block, false, &dii, &djj, &cvz, &gpu, SlowToFast,
                        &opz);
    bool thrown = false;
    try {
        const C *cxc = vxc;
        bsr_krylov<6, 6, 8, 8, C>(C(1), opz, "xyztsc", "XYZTSC", &px, 1, "pXYZTSCn", {{}}, dx, dx, &cxc,
                                  C(0), &px, "pxyztscn", {{}}, dx, dx, 'p', &vyc, &gpu, SlowToFast);
    } catch (const std::runtime_error &) { thrown = true; }
    CHECK(thrown, "complex<double> operator with complex<float> vectors throws std::runtime_error");
    std::vector<C> outc = download(vyc, nx);
    bool same = true;
    for (long i = 0; i < nx; ++i) same &= outc[i] == C(7);
    CHECK(same, "a refused call leaves y untouched");
    destroy_bsr(opz);

    deallocate(dv, gpu);
    deallocate(dvz, gpu);
    deallocate(dii, gpu);
    deallocate((IndexType *)djj, gpu);
    deallocate(vx, gpu);
    deallocate(vy, gpu);
    deallocate(vxc, gpu);
    deallocate(vyc, gpu);
    if (failures == 0) std::printf("mixed_bsr_test: all checks passed\n");
    return failures ? 1 : 0;
}
