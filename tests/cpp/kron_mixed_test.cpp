// Mixed-precision Kronecker operators through the drop-in header (include/superbblas.h),
// compiled with plain g++: an operator of create_kron_bsr<6, 6, std::complex<float>> (colour
// blocks and spin matrices in complex<float>) contracted by
// bsr_krylov<6, 6, 8, 8, std::complex<double>> on the same handle under
// sbx_tune_set("bsr.kron_mixed", 1): A x (x with the domain labels) and A^H x (x with the image
// labels) against host loops in double on the widened values.  Integers of magnitude at most 6
// and 45 terms per output of the 3x3 (x) 4x4 operator with five nonzeros per row: every sum is
// exact in any order.  With the key at 0 (the default) the same call must throw
// std::runtime_error and leave y as it was.
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
    // 3^4 lattice, 3x3 colour blocks (x) 4x4 spin matrices, five nonzeros per row: the site and
    // its forward neighbour in each direction
    const int L = 3, s = 4, c = 3, nb = 5, nc = 5;
    const Coor<6> dim{L, L, L, L, s, c};
    const long V = (long)L * L * L * L;
    std::vector<IndexType> ii(V, nb);
    std::vector<Coor<6>> jj;
    std::vector<long> site(V * nb);
    for (long i = 0; i < V; ++i) {
        Coor<6> cc{(int)(i / (L * L * L)), (int)(i / (L * L) % L), (int)(i / L % L), (int)(i % L), 0, 0};
        jj.push_back(cc);
        for (int d = 0; d < 4; ++d) {
            Coor<6> q = cc;
            q[d] = (q[d] + 1) % L;
            jj.push_back(q);
        }
        for (int k = 0; k < nb; ++k) {
            const Coor<6> &q = jj[i * nb + k];
            site[i * nb + k] = ((q[0] * L + q[1]) * L + q[2]) * L + q[3];
        }
    }
    // colour blocks U(k)(i, d) and spin matrices K(mu)(a, b), row major, in complex<float>
    const long nv = V * nb * c * c, nk = (long)nb * s * s;
    std::vector<C> hv(nv), hk(nk);
    for (long i = 0; i < nv; ++i) hv[i] = C((float)re_of(i, 4), (float)im_of(i, 4));
    for (long i = 0; i < nk; ++i) hk[i] = C((float)re_of(i, 2), (float)im_of(i, 2));
    // vectors (site, colour, column, spin) in complex<double>
    const Coor<8> dx{1, L, L, L, L, c, nc, s};
    const long nx = V * c * nc * s;
    std::vector<Z> hx(nx), hy(nx, Z(7));
    for (long i = 0; i < nx; ++i) hx[i] = Z(re_of(i, 5), im_of(i, 5));

    const C *dv = upload(hv), *dk = upload(hk);
    IndexType *dii = upload(ii);
    std::vector<IndexType> jflat((const IndexType *)jj.data(), (const IndexType *)jj.data() + jj.size() * 6);
    Coor<6> *djj = (Coor<6> *)upload(jflat);
    Z *vx = upload(hx), *vy = upload(hy);
    const Z *cx = vx;

    PartitionItem<6> pop{Coor<6>{}, dim};
    PartitionItem<8> px{Coor<8>{}, dx};
    const Coor<6> block{1, 1, 1, 1, 1, c}, kron{1, 1, 1, 1, s, 1};
    BSR_handle *op = nullptr;
    create_kron_bsr<6, 6, C>(&pop, dim, &pop, dim, 1, block, block, kron, kron, false, &dii, &djj, &dv,
                             &dk, &gpu, SlowToFast, &op);

    // the key at 0 (the default): the pair is refused and y keeps its values
    long long key = -1;
    CHECK(sbx_tune_get("bsr.kron_mixed", &key) == 0 && key == 0, "bsr.kron_mixed is 0 by default");
    bool thrown = false;
    try {
        bsr_krylov<6, 6, 8, 8, Z>(Z(1), op, "xyztsc", "XYZTSC", &px, 1, "pXYZTCnS", {{}}, dx, dx, &cx,
                                  Z(0), &px, "pxyztcns", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    } catch (const std::runtime_error &) { thrown = true; }
    CHECK(thrown, "complex<float> Kronecker operator with complex<double> vectors throws at key 0");
    std::vector<Z> out = download(vy, nx);
    bool same = true;
    for (long i = 0; i < nx; ++i) same &= out[i] == Z(7);
    CHECK(same, "a refused call leaves y untouched");

    // the key at 1: A x
    CHECK(sbx_tune_set("bsr.kron_mixed", 1) == 0, "bsr.kron_mixed can be set");
    auto at = [&](long st, int col, int sp, int n) { return ((st * c + col) * nc + n) * s + sp; };
    const Z alpha(2, -1);
    bsr_krylov<6, 6, 8, 8, Z>(alpha, op, "xyztsc", "XYZTSC", &px, 1, "pXYZTCnS", {{}}, dx, dx, &cx, Z(0),
                              &px, "pxyztcns", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    long long mixed = -1;
    CHECK(sbx_tune_get("bsr.last_mixed", &mixed) == 0 && mixed == 1, "bsr.last_mixed reads 1");
    out = download(vy, nx);
    bool ok = true;
    for (long r = 0; r < V; ++r)
        for (int i = 0; i < c; ++i)
            for (int n = 0; n < nc; ++n)
                for (int a = 0; a < s; ++a) {
                    Z acc = 0;
                    for (int k = 0; k < nb; ++k)
                        for (int d = 0; d < c; ++d)
                            for (int b = 0; b < s; ++b)
                                acc += Z(hk[(k * s + a) * s + b]) * Z(hv[((r * nb + k) * c + i) * c + d]) *
                                       hx[at(site[r * nb + k], d, b, n)];
                    ok &= out[at(r, i, a, n)] == alpha * acc;
                }
    CHECK(ok, "A x: complex<float> Kronecker operator, complex<double> vectors");

    // A^H x: x with the image labels
    bsr_krylov<6, 6, 8, 8, Z>(alpha, op, "xyztsc", "XYZTSC", &px, 1, "pxyztcns", {{}}, dx, dx, &cx, Z(0),
                              &px, "pXYZTCnS", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    out = download(vy, nx);
    std::vector<Z> ref(nx, Z(0));
    for (long r = 0; r < V; ++r)
        for (int k = 0; k < nb; ++k)
            for (int i = 0; i < c; ++i)
                for (int d = 0; d < c; ++d)
                    for (int a = 0; a < s; ++a)
                        for (int b = 0; b < s; ++b)
                            for (int n = 0; n < nc; ++n)
                                ref[at(site[r * nb + k], d, b, n)] +=
                                    std::conj(Z(hk[(k * s + a) * s + b]) * Z(hv[((r * nb + k) * c + i) * c + d])) *
                                    hx[at(r, i, a, n)];
    ok = true;
    for (long i = 0; i < nx; ++i) ok &= out[i] == alpha * ref[i];
    CHECK(ok, "A^H x: complex<float> Kronecker operator, complex<double> vectors");
    sbx_tune_set("bsr.kron_mixed", 0);
    destroy_bsr(op);

    deallocate((C *)dv, gpu);
    deallocate((C *)dk, gpu);
    deallocate(dii, gpu);
    deallocate((IndexType *)djj, gpu);
    deallocate(vx, gpu);
    deallocate(vy, gpu);
    if (failures == 0) std::printf("kron_mixed_test: all checks passed\n");
    return failures ? 1 : 0;
}
