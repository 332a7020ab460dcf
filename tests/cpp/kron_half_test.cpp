// Half-precision Kronecker operators through the drop-in header (include/superbblas.h),
// compiled with plain g++ (no _Float16 needed): an operator of
// create_kron_bsr<6, 6, superbblas::complex_float16> (colour blocks and spin matrices in IEEE
// binary16, re and im) contracted by bsr_krylov<6, 6, 8, 8, std::complex<float>> on the same
// handle under sbx_tune_set("bsr.kron_half", 1): A x (x with the domain labels) and A^H x (x with
// the image labels) against host loops in double on the widened values.  Integers of magnitude at
// most 6 and 60 terms per output of the 3x3 (x) 4x4 operator with five nonzeros per row: a
// component of K U is at most 2 * 36, of K U x 2 * 72 * 6, so every partial sum, alpha (2 - i)
// included, is an integer below 60 * 864 * 3 < 2^18: exact in float in any order.
// With the key at 0 (the default) the creation must throw std::runtime_error; with the key at 1 a
// std::complex<double> call on the handle must throw and leave y as it was.
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
// the library copies no half tensors: the 4-byte values travel as the ints of their bits
static const H *upload_half(const std::vector<H> &h) {
    static_assert(sizeof(H) == sizeof(int), "a complex_float16 is one int of bits");
    std::vector<int> bits(h.size());
    std::memcpy(bits.data(), h.data(), h.size() * sizeof(int));
    return (const H *)upload(bits);
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
    // colour blocks U(k)(i, d) and spin matrices K(mu)(a, b), row major: as complex_float16 and,
    // widened, as complex<double> for the host loops
    const long nv = V * nb * c * c, nk = (long)nb * s * s;
    std::vector<H> hv(nv), hk(nk);
    std::vector<Z> wv(nv), wk(nk);
    for (long i = 0; i < nv; ++i) {
        hv[i] = H{half_of(re_of(i, 4)), half_of(im_of(i, 4))};
        wv[i] = Z(re_of(i, 4), im_of(i, 4));
    }
    for (long i = 0; i < nk; ++i) {
        hk[i] = H{half_of(re_of(i, 2)), half_of(im_of(i, 2))};
        wk[i] = Z(re_of(i, 2), im_of(i, 2));
    }
    // vectors (site, colour, column, spin) in complex<float>, and in complex<double> for the refusal
    const Coor<8> dx{1, L, L, L, L, c, nc, s};
    const long nx = V * c * nc * s;
    std::vector<C> hx(nx), hy(nx, C(7));
    std::vector<Z> hxz(nx), hyz(nx, Z(7));
    for (long i = 0; i < nx; ++i) {
        hx[i] = C((float)re_of(i, 5), (float)im_of(i, 5));
        hxz[i] = Z(re_of(i, 5), im_of(i, 5));
    }

    const H *dv = upload_half(hv), *dk = upload_half(hk);
    IndexType *dii = upload(ii);
    std::vector<IndexType> jflat((const IndexType *)jj.data(), (const IndexType *)jj.data() + jj.size() * 6);
    Coor<6> *djj = (Coor<6> *)upload(jflat);
    C *vx = upload(hx), *vy = upload(hy);
    Z *vxz = upload(hxz), *vyz = upload(hyz);
    const C *cx = vx;
    const Z *cxz = vxz;

    PartitionItem<6> pop{Coor<6>{}, dim};
    PartitionItem<8> px{Coor<8>{}, dx};
    const Coor<6> block{1, 1, 1, 1, 1, c}, kron{1, 1, 1, 1, s, 1};
    BSR_handle *op = nullptr;

    // the key at 0 (the default): the creation is refused
    long long key = -1;
    CHECK(sbx_tune_get("bsr.kron_half", &key) == 0 && key == 0, "bsr.kron_half is 0 by default");
    bool thrown = false;
    try {
        create_kron_bsr<6, 6, H>(&pop, dim, &pop, dim, 1, block, block, kron, kron, false, &dii, &djj, &dv,
                                 &dk, &gpu, SlowToFast, &op);
    } catch (const std::runtime_error &) { thrown = true; }
    CHECK(thrown && op == nullptr, "create_kron_bsr<complex_float16> throws at key 0");

    // the key at 1: the creation, then A x
    CHECK(sbx_tune_set("bsr.kron_half", 1) == 0, "bsr.kron_half can be set");
    create_kron_bsr<6, 6, H>(&pop, dim, &pop, dim, 1, block, block, kron, kron, false, &dii, &djj, &dv, &dk,
                             &gpu, SlowToFast, &op);
    auto at = [&](long st, int col, int sp, int n) { return ((st * c + col) * nc + n) * s + sp; };
    const C alpha(2, -1);
    const Z alphaz(2, -1);
    bsr_krylov<6, 6, 8, 8, C>(alpha, op, "xyztsc", "XYZTSC", &px, 1, "pXYZTCnS", {{}}, dx, dx, &cx, C(0),
                              &px, "pxyztcns", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    long long mixed = -1;
    CHECK(sbx_tune_get("bsr.last_mixed", &mixed) == 0 && mixed == 1, "bsr.last_mixed reads 1");
    std::vector<C> out = download(vy, nx);
    bool ok = true;
    for (long r = 0; r < V; ++r)
        for (int i = 0; i < c; ++i)
            for (int n = 0; n < nc; ++n)
                for (int a = 0; a < s; ++a) {
                    Z acc = 0;
                    for (int k = 0; k < nb; ++k)
                        for (int d = 0; d < c; ++d)
                            for (int b = 0; b < s; ++b)
                                acc += wk[(k * s + a) * s + b] * wv[((r * nb + k) * c + i) * c + d] *
                                       hxz[at(site[r * nb + k], d, b, n)];
                    ok &= Z(out[at(r, i, a, n)]) == alphaz * acc;
                }
    CHECK(ok, "A x: complex_float16 Kronecker operator, complex<float> vectors");

    // A^H x: x with the image labels
    bsr_krylov<6, 6, 8, 8, C>(alpha, op, "xyztsc", "XYZTSC", &px, 1, "pxyztcns", {{}}, dx, dx, &cx, C(0),
                              &px, "pXYZTCnS", {{}}, dx, dx, 'p', &vy, &gpu, SlowToFast);
    long long kernel = -1;
    CHECK(sbx_tune_get("bsr.last_kernel", &kernel) == 0 && kernel == 15, "bsr.last_kernel reads 15 for A^H");
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
                                    std::conj(wk[(k * s + a) * s + b] * wv[((r * nb + k) * c + i) * c + d]) *
                                    hxz[at(r, i, a, n)];
    ok = true;
    for (long i = 0; i < nx; ++i) ok &= Z(out[i]) == alphaz * ref[i];
    CHECK(ok, "A^H x: complex_float16 Kronecker operator, complex<float> vectors");

    // complex<double> vectors stay refused, y untouched
    thrown = false;
    try {
        bsr_krylov<6, 6, 8, 8, Z>(Z(1), op, "xyztsc", "XYZTSC", &px, 1, "pXYZTCnS", {{}}, dx, dx, &cxz, Z(0),
                                  &px, "pxyztcns", {{}}, dx, dx, 'p', &vyz, &gpu, SlowToFast);
    } catch (const std::runtime_error &) { thrown = true; }
    CHECK(thrown, "complex_float16 Kronecker operator with complex<double> vectors throws");
    std::vector<Z> outz = download(vyz, nx);
    bool same = true;
    for (long i = 0; i < nx; ++i) same &= outz[i] == Z(7);
    CHECK(same, "a refused call leaves y untouched");

    sbx_tune_set("bsr.kron_half", 0);
    destroy_bsr(op);
    deallocate((int *)dv, gpu);
    deallocate((int *)dk, gpu);
    deallocate(dii, gpu);
    deallocate((IndexType *)djj, gpu);
    deallocate(vx, gpu);
    deallocate(vy, gpu);
    deallocate(vxz, gpu);
    deallocate(vyz, gpu);
    if (failures == 0) std::printf("kron_half_test: all checks passed\n");
    return failures ? 1 : 0;
}
