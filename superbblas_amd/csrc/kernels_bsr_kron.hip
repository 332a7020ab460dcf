// Kronecker BSR operator times dense tensor (the Wilson-type stencil: a color block per
// direction times a spin matrix shared by all sites of that direction).
//
// Reference: create_kron_bsr (bsr.h:2476-2490), get_kron_indices (bsr.h:1485-1537), the builtin
// CPU operator (bsr.h:587-648) and BSR<Gpu>::contract_kron_cols + hipsparseXbsrmm
// (bsr.h:933-998, 1001-1029):
//   y(I, i, n, a) = alpha * sum_mu sum_b K_mu(a, b) sum_d U_{I,mu}(i, d) x(J(I,mu), d, n, b)
// with mu the position of the nonzero within its block row (every row has the same count).
// Layout (row major, SlowToFast): x (site, d, n, b), y (site, i, n, a): one thread per
// (block row, rhs column) owns the bi*ki outputs of that pair, reads bd*kd contiguous x values
// per neighbour (consecutive lanes -> consecutive rhs columns -> contiguous 16*kd-byte pieces),
// and the spin matrix K_mu is wave-uniform (scalar loads; zero entries -- half of a Wilson
// projector -- are skipped with a scalar branch).
#include "elem_ops.h"
#include "kernel_util.h"
#include "sbx_internal.h"

#include <algorithm>
#include <type_traits>

namespace sbx {
namespace {

struct KronArgs {
    long block_rows;
    int nnz; ///< nonzero blocks per block row
    int bi, bd, ki, kd;
    const int *jj; ///< domain site of nonzero r*nnz + mu
    const void *v;
    const void *kron;
    int block_im_fast;
    const void *x;
    void *y;
    long ncols;
    double alpha_re, alpha_im;
    int add;
    int ylds; ///< the XL kernels: y written through the wave's LDS ring in whole 64-B spin pieces
    long x_rows; ///< domain rows of x (sites * bd): the extent x's LDS-DMA buffer offsets address
    const int *perm; ///< the spin-first kernel: block row of each row slot (nullptr: the identity)
    const void *ktab; ///< ... the spin matrices' rows as two terms (bsr.cpp build_kron_terms)
    const void *xtab; ///< ... as diagonal + XOR partner (nullptr: not of that form)
};

/// The epilogue of a lane that owns NI x NA outputs of y (., i, n, a) at column c, ys = &y(., 0, c, 0):
/// y(i, a) = alpha acc(i, a) [+ y(i, a)], acc(i, a) the lane's sum as an E
template <typename E, int NI, int NA, typename Acc>
__device__ __forceinline__ void store_outputs(E *ys, long n, double alpha_re, double alpha_im, int add, Acc acc) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            E o = Ops<E>::scale(acc(i, a), alpha_re, alpha_im);
            if (add) o = Ops<E>::add(o, ys[i * n * NA + a]);
            ys[i * n * NA + a] = o;
        }
}

// Mixed precision (bsr.kron_mixed): every kernel of this file but the spin-first ones has a value
// type EV beside the vector type E -- EV = E, or float / float2 under double / double2.  The
// colour blocks v and the spin matrices kron are read in place as EV and widened (to_vec, exact)
// where they are read; x, y, products, sums and alpha are E.  No converted copy exists.
// Half precision (bsr.kron_half): the same one step down, EV = f16 / f16x2 under float / float2,
// on the VALU kernels (the matrix-core forms are complex<double> vectors only).
template <typename EV, typename E, int BI, int BD, int KI, int KD>
__global__ void __launch_bounds__(256) bsr_kron_kernel(const KronArgs p) {
    const EV *__restrict__ v = (const EV *)p.v;
    const EV *__restrict__ kron = (const EV *)p.kron;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const long total = p.block_rows * p.ncols;
    const long xsite = (long)BD * p.ncols * KD, xrow = p.ncols * KD;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
        const long c = idx % p.ncols, r = idx / p.ncols;
        E acc[BI][KI];
#pragma unroll
        for (int i = 0; i < BI; ++i)
#pragma unroll
            for (int a = 0; a < KI; ++a) acc[i][a] = Ops<E>::zero();
        for (int mu = 0; mu < p.nnz; ++mu) {
            const long j = r * p.nnz + mu;
            const E *xs = x + p.jj[j] * xsite + c * KD;
            E xv[BD][KD];
#pragma unroll
            for (int d = 0; d < BD; ++d)
#pragma unroll
                for (int b = 0; b < KD; ++b) xv[d][b] = xs[d * xrow + b];
            // spin first: xk(d, a) = sum_b K_mu(a, b) x(d, b)
            const EV *K = kron + (long)mu * KI * KD;
            E xk[BD][KI];
#pragma unroll
            for (int d = 0; d < BD; ++d)
#pragma unroll
                for (int a = 0; a < KI; ++a) xk[d][a] = Ops<E>::zero();
#pragma unroll
            for (int a = 0; a < KI; ++a)
#pragma unroll
                for (int b = 0; b < KD; ++b) {
                    const E k = to_vec<E>(p.block_im_fast ? K[a + b * KI] : K[a * KD + b]);
                    if (!Ops<E>::nonzero(k)) continue;
#pragma unroll
                    for (int d = 0; d < BD; ++d) xk[d][a] = Ops<E>::fma(k, xv[d][b], xk[d][a]);
                }
            // color: acc(i, a) += sum_d U(i, d) xk(d, a)
            const EV *U = v + j * BI * BD;
#pragma unroll
            for (int i = 0; i < BI; ++i)
#pragma unroll
                for (int d = 0; d < BD; ++d) {
                    const E u = to_vec<E>(p.block_im_fast ? U[i + d * BI] : U[i * BD + d]);
#pragma unroll
                    for (int a = 0; a < KI; ++a) acc[i][a] = Ops<E>::fma(u, xk[d][a], acc[i][a]);
                }
        }
        store_outputs<E, BI, KI>(y + (r * BI * p.ncols + c) * KI, p.ncols, p.alpha_re, p.alpha_im, p.add,
                                 [&](int i, int a) { return acc[i][a]; });
    }
}

/// Bytes of bsr_kron_lds_kernel's LDS image of `nvalues` values of EV, a multiple of 4: the block
/// columns (ints) follow it
template <typename EV> constexpr long kron_lds_values_bytes(long nvalues) {
    return (nvalues * (long)sizeof(EV) + 3) / 4 * 4;
}

/// Many rhs columns: a workgroup owns `S` consecutive block rows x up to 256 columns; the color
/// blocks of its rows (S * NNZ * BI * BD values, contiguous in memory) and their domain sites are
/// staged in LDS with coalesced loads (instead of every lane of a row fetching the same 9 blocks
/// through L1), the spin matrices are read through the constant address space so that they live
/// in SGPRs (wave-uniform operands of the FMAs), and the x values of the next nonzero are loaded
/// while the current one is being applied (the loop over the NNZ nonzeros is unrolled).
/// Mixed: the LDS image Us holds the values as stored (EV: half the LDS), widened at the LDS read;
/// the spin matrices are scalar loads of EV, widened on the scalar side's way into the FMAs.
/// 2-byte values (f16 under float): S * BLK of them are an odd number of halves for odd S (5, 10
/// and 17 columns: S = 51, 25, 15), so the values' image is padded to whole dwords and Js stays
/// 4-byte aligned (kron_lds_values_bytes: the kernel's and the launcher's one statement of it).
/// The staging is one element per load: exact at both ends of the run for a value array that is
/// only element-aligned and that ends with the last row's last value.
template <typename EV, typename E, int BI, int BD, int KI, int KD, int NNZ>
__global__ void __launch_bounds__(256) bsr_kron_lds_kernel(const KronArgs p, int S, int cpg) {
    extern __shared__ char smem[];
    constexpr int BLK = BI * BD * NNZ;
    EV *Us = (EV *)smem;
    int *Js;
    if constexpr (sizeof(EV) % 4 == 0) Js = (int *)(Us + (long)S * BLK);
    else Js = (int *)(smem + kron_lds_values_bytes<EV>((long)S * BLK));
    const EV *__restrict__ v = (const EV *)p.v;
    const EV *kron = (const EV *)p.kron;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    // consecutive chunks of block rows on one XCD: neighbouring sites share x lines in its L2
    const int wg = xcd_chunk(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int gx = wg % gridDim.x, gy = wg / gridDim.x;
    const long r0 = (long)gx * S;
    const int nrows = (int)std::min<long>(S, p.block_rows - r0);
    {
        const EV *src = v + r0 * BLK;
        for (int e = threadIdx.x; e < nrows * BLK; e += 256) Us[e] = src[e];
        const int *jsrc = p.jj + r0 * NNZ;
        for (int e = threadIdx.x; e < nrows * NNZ; e += 256) Js[e] = jsrc[e];
    }
    __syncthreads();
    const int sl = threadIdx.x / cpg;
    const long c = (long)gy * cpg + threadIdx.x % cpg;
    if (sl >= nrows || c >= p.ncols) return;
    const long r = r0 + sl;
    const long xsite = (long)BD * p.ncols * KD, xrow = p.ncols * KD;
    const E *xc = x + c * KD;
    E acc[BI][KI];
#pragma unroll
    for (int i = 0; i < BI; ++i)
#pragma unroll
        for (int a = 0; a < KI; ++a) acc[i][a] = Ops<E>::zero();
    const EV *Ur = Us + sl * BLK;
    const int *Jr = Js + sl * NNZ;
    E xa[BD][KD];
    {
        const E *xs = xc + Jr[0] * xsite;
#pragma unroll
        for (int d = 0; d < BD; ++d)
#pragma unroll
            for (int b = 0; b < KD; ++b) xa[d][b] = xs[d * xrow + b];
    }
#pragma unroll 1
    for (int mu = 0; mu < NNZ; ++mu) {
        E xb[BD][KD];
        if (mu + 1 < NNZ) {
            const E *xs = xc + Jr[mu + 1] * xsite;
#pragma unroll
            for (int d = 0; d < BD; ++d)
#pragma unroll
                for (int b = 0; b < KD; ++b) xb[d][b] = xs[d * xrow + b];
        }
        const EV *K = kron + mu * KI * KD;
        const EV *U = Ur + mu * BI * BD;
#pragma unroll
        for (int d = 0; d < BD; ++d) {
            // spin: xk(a) = sum_b K_mu(a, b) x(d, b)
            E xk[KI];
#pragma unroll
            for (int a = 0; a < KI; ++a) {
                xk[a] = Ops<E>::zero();
#pragma unroll
                for (int b = 0; b < KD; ++b)
                    xk[a] = Ops<E>::fma(
                        to_vec<E>(Uniform<EV>::load(K, p.block_im_fast ? a + b * KI : a * KD + b)),
                        xa[d][b], xk[a]);
            }
            // color: acc(i, a) += U(i, d) xk(a)
#pragma unroll
            for (int i = 0; i < BI; ++i) {
                const E u = to_vec<E>(p.block_im_fast ? U[i + d * BI] : U[i * BD + d]);
#pragma unroll
                for (int a = 0; a < KI; ++a) acc[i][a] = Ops<E>::fma(u, xk[a], acc[i][a]);
            }
        }
        if (mu + 1 < NNZ) {
#pragma unroll
            for (int d = 0; d < BD; ++d)
#pragma unroll
                for (int b = 0; b < KD; ++b) xa[d][b] = xb[d][b];
        }
    }
    store_outputs<E, BI, KI>(y + (r * BI * p.ncols + c) * KI, p.ncols, p.alpha_re, p.alpha_im, p.add,
                             [&](int i, int a) { return acc[i][a]; });
}

/// Any block / Kronecker sizes: one thread per output element (block row, i, column, a)
template <typename EV, typename E>
__global__ void __launch_bounds__(256) bsr_kron_generic_kernel(const KronArgs p) {
    const EV *__restrict__ v = (const EV *)p.v;
    const EV *__restrict__ kron = (const EV *)p.kron;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const long total = p.block_rows * p.bi * p.ncols * p.ki;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
        const int a = (int)(idx % p.ki);
        long t = idx / p.ki;
        const long c = t % p.ncols;
        t /= p.ncols;
        const int i = (int)(t % p.bi);
        const long r = t / p.bi;
        E acc = Ops<E>::zero();
        for (int mu = 0; mu < p.nnz; ++mu) {
            const long j = r * p.nnz + mu;
            const E *xs = x + (long)p.jj[j] * p.bd * p.ncols * p.kd + c * p.kd;
            const EV *K = kron + (long)mu * p.ki * p.kd;
            const EV *U = v + j * p.bi * p.bd;
            for (int b = 0; b < p.kd; ++b) {
                const E k = to_vec<E>(p.block_im_fast ? K[a + b * p.ki] : K[a * p.kd + b]);
                if (!Ops<E>::nonzero(k)) continue;
                E s = Ops<E>::zero();
                for (int d = 0; d < p.bd; ++d) {
                    const E u = to_vec<E>(p.block_im_fast ? U[i + d * p.bi] : U[i * p.bd + d]);
                    s = Ops<E>::fma(u, xs[d * p.ncols * p.kd + b], s);
                }
                acc = Ops<E>::fma(k, s, acc);
            }
        }
        E o = Ops<E>::scale(acc, p.alpha_re, p.alpha_im);
        if (p.add) o = Ops<E>::add(o, y[idx]);
        y[idx] = o;
    }
}

// complex<double> vectors, 3x3 color blocks, 4x4 spin matrices, from 8 rhs columns, on the matrix
// cores: bsr_kron_mfma_kernel (form 5) and bsr_kron_mfma_packed_kernel (form 6).  A wave owns 16
// column slots of a block row (form 6: of several rows), lane l = 16 b + q owning spin b of slot q.
//  * color on the VALU: T_mu(i, b, q) = sum_d U_mu(i, d) x(J_mu, d, q, b) -- the color blocks of
//    the workgroup's rows are one contiguous run of the value array, staged in LDS once and
//    read back as broadcasts;
//  * spin on the matrix cores: acc(a, i, q) += sum_b K_mu(a, b) T_mu(i, b, q) is a 4x4x4 product
//    per group of 4 slots, i.e. v_mfma_f64_4x4x4_4b_f64 with A = K_mu (lane 16 b + 4 g + a, the
//    same in all 4 blocks), B = T (lane 16 b + q) and C = acc (lane 16 a + q) -- the lane maps
//    measured by tools/mfma_small.hip -- 4 real products per complex one (the BLAS rounding);
//  * XL = 0: the next neighbour's x is loaded into VGPRs while the current one is applied (per
//    lane: 3 loads of 16 bytes, lane-linear over the columns of one spin);
//  * XL > 0: the neighbours' x pieces staged by LDS-DMA instead.  The MFMA's B operand wants lane
//    16 b + q = spin b of slot q, but spin is the fastest index of x in memory, so a 16-lane
//    quarter of such a load touches 16 pieces 64 B apart (8 cache lines; 32 TA/TCP accesses per
//    1-KB instruction against 8 for a linear one, and TA/TD busy 85-92 %).  The DMA instead moves
//    each slot's 4 spins as one 64-B piece (lane l: slot l / 4), writes them lane-linear into the
//    wave's ring (XL neighbours ahead, 3 KB per neighbour: deeper prefetch costs LDS, not VGPRs),
//    and the B lanes read them back with the spins rotated (position 4 q + (b + q / 2 + q / 8)
//    mod 4: the 16-B granules of any 8 or 16 lanes reading together fall on distinct banks).  The
//    spin matrices then sit in LDS too: no vector-memory load in the main loop, where the
//    compiler's own vmcnt waits (blind to the DMAs) would drain the x ring;
//  * p.ylds (XL > 0): y leaves through the same ring, each slot's 4 spins one 64-B run.
// EV = float2 (complex<float> values under complex<double> vectors, bsr.kron_mixed): only the
// colour run and the spin operand's source change.  The run sits in LDS as stored (8-byte values,
// half the LDS) and is widened at the LDS read; it is staged by plain 8-byte loads and LDS
// writes, not by LDS-DMA: the DMA moves 16-byte pieces, and a run of 8-byte values starts at
// row * 81 * 8 bytes of a tensor that is itself only 8-byte aligned -- no multiple of 16 for an odd
// first row (form 5 at 40 columns: ngroups 3, first row floor(4 wgi / 3)) or an odd base (form 6:
// the first row is even, the base need not be).  The loads are bounded by the run (e < nu), so
// nothing past the value array is read, whatever its alignment or length; at most two loads a
// lane, once per workgroup, before the x ring starts.  The spin matrices are widened where the
// ks image is filled (XL) or where they are loaded.
//
// One kernel (bsr_kron_mfma_form_kernel), two maps from lanes to (row, column) (PACK: false is
// bsr_kron_mfma_kernel, true bsr_kron_mfma_packed_kernel), everything else once -- and in the
// kernel's own text, not in helper functions: the compiler simplifies a helper before it inlines
// it, and this loop unrolled inside one, with the lane's data behind references, compiled to
// 90-190 instructions more and to other register counts.
//  * !PACK (form 5): 4 waves, wave w of workgroup wgi takes task 4 wgi + w of the (block row,
//    group of 16 columns) tasks, row-major over the a0 = ngroups groups.  The row is
//    wave-uniform, its block columns scalar loads where they are used; static LDS.
//  * PACK (form 6), rhs counts below 16 that divide 16 W (W <= 4 waves): the workgroup's 16 W
//    slots are the (row, column) pairs of its a0 = RW = 16 W / n consecutive block rows, so no
//    lane idles (at n = 12 one wave per row left 4 of 16 slots empty: 25 % of the VALU and MFMA
//    work).  The row is per lane: its block columns, and those of the DMA slot's row, are loaded
//    into registers up front.  Dynamic LDS: the color blocks of RW rows, from byte a1 the W
//    rings, then the spin matrices (the launcher sizes all three).
// XCD-contiguous workgroups, the XCD's range visited as two interleaved halves (the ilv form of
// the 3x3 kernels).  The kernel before these (one thread per (row, column) owning all 12 outputs)
// ran at 256 VGPRs: 2 waves per SIMD.
template <bool PACK, int NNZ, bool kpf = false, int XL = 0, typename EV = double2>
__global__ void __launch_bounds__(256) bsr_kron_mfma_form_kernel(const KronArgs p, int a0, int a1) {
    constexpr int NS = XL + 1;
    typedef double2 E;
    constexpr bool same = std::is_same<EV, E>::value;
    typedef typename BsrStored<EV, E>::type SV; // a value as stored: reading it as E widens
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nth = PACK ? (int)blockDim.x : 256;
    const long wgi = xcd_chunk(blockIdx.x, gridDim.x, 2);
    const long n = p.ncols;
    const int b = lane >> 4, q = lane & 15; // B and C operands: spin b of slot q
    // the DMA lane (x staged, y through the ring): the piece of slot lane / 4, its spin rotated back
    const int qd = lane >> 2, bd = ((lane & 3) - (qd >> 1) - (qd >> 3)) & 3;
    // the lane's output (r, col), if live; xcol: the column its x loads read; the DMA lane's slot
    // as an output (rowd, cold), if lived; the workgroup's run of color blocks: nu values from row0
    long r, col, xcol, rowd, cold, row0;
    bool live, lived;
    int nu;
    if constexpr (PACK) {
        row0 = wgi * a0;
        const int nrows = (int)min((long)a0, p.block_rows - row0);
        const int slot = w * 16 + q, rl = slot / (int)n;
        col = slot - (long)rl * n;
        live = rl < nrows;
        r = row0 + (live ? rl : nrows - 1);
        xcol = col;
        const int sd = w * 16 + qd, rld = sd / (int)n;
        cold = sd - (long)rld * n;
        lived = rld < nrows;
        rowd = row0 + (lived ? rld : nrows - 1);
        nu = nrows * NNZ * 9; // <= RW * NNZ * 9: the launcher's LDS for the run
    } else {
        const long task = wgi * 4 + w;
        r = task / a0;
        const int cg = (int)(task - r * a0);
        col = (long)cg * 16 + q;
        live = col < n;
        xcol = live ? col : n - 1;
        cold = (long)cg * 16 + qd;
        lived = cold < n;
        rowd = r;
        // a workgroup's 4 tasks span at most 4 rows, consecutive ones
        row0 = (wgi * 4) / a0;
        nu = (int)(min((wgi * 4 + 3) / a0, p.block_rows - 1) - row0 + 1) * NNZ * 9; // <= 4 * NNZ * 9
    }
    // LDS: the run, the spin matrices (XL), a ring of XL + 1 neighbours x 3 KB per wave (XL)
    extern __shared__ __attribute__((aligned(16))) char smem_k[];
    EV *us;
    E *ks, *ring;
    unsigned us_a, ring_a; // the LDS addresses of us and ring
    if constexpr (PACK) {
        const unsigned xring_w = (unsigned)a1 + (unsigned)w * (NS * 3072u);
        us = (EV *)smem_k, us_a = lds_u32(smem_k);
        ring = (E *)(smem_k + xring_w), ring_a = us_a + xring_w;
        ks = (E *)(smem_k + a1 + (nth >> 6) * NS * 3072);
    } else {
        // (the run rounded up to whole DMA passes of 256 lanes: the lanes past it write zeros)
        __shared__ __attribute__((aligned(16))) EV us_s[(4 * NNZ * 9 + 255) / 256 * 256];
        __shared__ __attribute__((aligned(16))) E ks_s[XL ? NNZ * 16 : 1];
        __shared__ __attribute__((aligned(16))) E xr_s[XL ? 4 * NS * 3 * 64 : 1];
        us = us_s, us_a = lds_u32(us_s), ks = ks_s;
        ring = xr_s + w * (NS * 192), ring_a = lds_u32(xr_s) + (unsigned)w * (NS * 3072u);
    }
    const SV *kron = (const SV *)p.kron;
    auto stage_spin = [&]() {
        for (int e = (int)threadIdx.x; e < NNZ * 16; e += nth) ks[e] = kron[e];
    };
    if constexpr (!PACK && XL > 0) stage_spin();
    // the run into LDS: one DMA pass per nth values (launcher: the value array is below 2 GiB), or
    // -- mixed -- plain loads bounded by the run; read back as broadcasts
    if constexpr (!same) {
        const EV *__restrict__ src = (const EV *)p.v + row0 * NNZ * 9;
        for (int e = (int)threadIdx.x; e < nu; e += nth) us[e] = src[e];
    } else {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)p.v, (short)0, (int)(p.block_rows * NNZ * 9 * 16), 0x00020000);
        const unsigned base = us_a + (unsigned)w * 1024u;
        for (int u = 0; u * nth < nu; ++u) {
            const int e = u * nth + (int)threadIdx.x;
            const unsigned off = e < nu ? (unsigned)(row0 * NNZ * 9 + e) * 16u : 0x80000000u;
            dma16(rs, off, base + (unsigned)(u * nth) * 16u);
        }
        if constexpr (!PACK) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if constexpr (!PACK) {
        __syncthreads();
        if (r >= p.block_rows) return;
    }
    // block columns of the lane's row and of its DMA slot's row: registers (PACK) or scalar loads
    int jrow_v[PACK ? NNZ : 1], jd_v[PACK && XL > 0 ? NNZ : 1];
    const ConstPtr<int> jrow_s = (ConstPtr<int>)(p.jj + r * NNZ);
    auto jcol = [&](int mu) { // block column mu of the lane's row
        if constexpr (PACK) return jrow_v[mu];
        else return jrow_s[mu];
    };
    auto jdcol = [&](int mu) { // ... of the DMA slot's row
        if constexpr (PACK) return jd_v[mu];
        else return jrow_s[mu];
    };
    if constexpr (PACK) {
#pragma unroll
        for (int mu = 0; mu < NNZ; ++mu) jrow_v[mu] = p.jj[r * NNZ + mu];
        if constexpr (XL > 0) {
#pragma unroll
            for (int mu = 0; mu < NNZ; ++mu) jd_v[mu] = p.jj[rowd * NNZ + mu];
        }
    }
    // spin matrices as the A operand: lane 16 k + 4 g + a holds K_mu(a, k)
    const int ka = lane & 3, kk = lane >> 4;
    const int kidx = p.block_im_fast ? ka + kk * 4 : ka * 4 + kk;
    const long xsite = 3 * n * 4; // elements per domain site: (d, n, b)
    auto load_x = [&](int J, E *xv) {
        const E *xs = x + (long)J * xsite + xcol * 4 + b;
#pragma unroll
        for (int d = 0; d < 3; ++d) xv[d] = xs[d * n * 4];
    };
    E xa[3], xb[3];
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)x, (short)0, 0x7fffffff, 0x00020000);
    const unsigned xoff_d = (unsigned)((PACK ? cold : min(cold, n - 1)) * 4 + bd) * 16u;
    if constexpr (PACK && XL > 0) {
        stage_spin();
        // the DMA lanes' block columns: consumed here, so that no load of them is pending
        // (and waited for by the compiler) inside the loop
#pragma unroll
        for (int mu = 0; mu < NNZ; ++mu) asm volatile("" : "+v"(jd_v[mu]));
    }
    auto issue_x = [&](int mu) {
        const unsigned base = ring_a + (unsigned)(mu % NS) * 3072u;
        const unsigned o = (unsigned)((long)jdcol(mu) * xsite) * 16u + xoff_d;
#pragma unroll
        for (int d = 0; d < 3; ++d) dma16(rx, o + (unsigned)(d * n * 4) * 16u, base + (unsigned)d * 1024u);
    };
    // the B lane's position in a ring slot
    const int xpos = 4 * q + ((b + (q >> 1) + (q >> 3)) & 3);
    if constexpr (XL > 0) {
#pragma unroll
        for (int mu = 0; mu < XL && mu < NNZ; ++mu) issue_x(mu);
    } else {
        load_x(jcol(0), xa);
    }
    if constexpr (PACK) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const SV *urow_s = (const SV *)us + (r - row0) * NNZ * 9;
    double accR[3] = {0, 0, 0}, accI[3] = {0, 0, 0};
    // the spin matrix of neighbour mu + 1 is loaded with its x rows; the compiler barrier keeps
    // the unrolled loop from hoisting all 9 spin-matrix loads to the top (36 more VGPRs: fewer
    // waves per SIMD)
    E Kc = XL > 0 ? E{} : E(kron[kidx]);
#pragma unroll
    for (int mu = 0; mu < NNZ; ++mu) {
        if constexpr (kpf) asm volatile("" ::: "memory");
        E Kn = Kc;
        if constexpr (XL > 0) {
            // the ring slot of neighbour mu + XL was read in iteration mu - 1: those reads are done
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (mu + XL < NNZ) issue_x(mu + XL);
            // neighbour mu landed: its successors' DMAs (and the next spin load) may stay in flight
            wait_vmcnt(3 * (NNZ - 1 - mu < XL ? NNZ - 1 - mu : XL));
            const E *xs = ring + (mu % NS) * 192;
#pragma unroll
            for (int d = 0; d < 3; ++d) xa[d] = xs[d * 64 + xpos];
        } else if (mu + 1 < NNZ) {
            load_x(jcol(mu + 1), xb);
            if constexpr (kpf) Kn = kron[(mu + 1) * 16 + kidx];
        }
        const E K = XL > 0 ? ks[mu * 16 + kidx] : kpf ? Kc : E(kron[mu * 16 + kidx]);
        Kc = Kn;
        // color: T(i) = sum_d U(i, d) x(d)
        E t[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t[i] = Ops<E>::zero();
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const long ui = mu * 9 + (p.block_im_fast ? i + d * 3 : i * 3 + d);
                t[i] = Ops<E>::fma(urow_s[ui], xa[d], t[i]);
            }
        }
        // spin: acc(a) += K(a, b) T(b) on the matrix cores, 4 real products per complex one
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            accR[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(K.x, t[i].x, accR[i], 0, 0, 0);
            accR[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(-K.y, t[i].y, accR[i], 0, 0, 0);
            accI[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(K.x, t[i].y, accI[i], 0, 0, 0);
            accI[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(K.y, t[i].x, accI[i], 0, 0, 0);
        }
        if (XL == 0 && mu + 1 < NNZ) {
#pragma unroll
            for (int d = 0; d < 3; ++d) xa[d] = xb[d];
        }
    }
    if constexpr (XL > 0) {
        if (p.ylds) {
            // C lane 16 a + q -> ring position xpos (the B read's map, a in place of b); then
            // lane l stores the piece of slot l / 4: each slot's 4 spins one 64-B run
            E *ys = ring;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                ys[i * 64 + xpos] = Ops<E>::scale(E{accR[i], accI[i]}, p.alpha_re, p.alpha_im);
            asm volatile("" ::: "memory");
            if (!lived) return;
            const long rs = PACK ? row0 + (w * 16 + qd) / (int)n : r;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                E *yp = y + ((rs * 3 + i) * n + cold) * 4 + bd;
                E o = ys[i * 64 + lane];
                if (p.add) o = Ops<E>::add(o, *yp);
                *yp = o;
            }
            return;
        }
    }
    if (!live) return;
    // C lane 16 a + q: spin a of slot q
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        E *yp = y + ((r * 3 + i) * n + col) * 4 + b;
        E o = Ops<E>::scale(E{accR[i], accI[i]}, p.alpha_re, p.alpha_im);
        if (p.add) o = Ops<E>::add(o, *yp);
        *yp = o;
    }
}

/// The two forms by the names the launcher, the tests and the documents know them by
template <int NNZ, bool kpf, int XL, typename EV>
constexpr auto *bsr_kron_mfma_kernel = &bsr_kron_mfma_form_kernel<false, NNZ, kpf, XL, EV>;
template <int NNZ, bool kpf, int XL, typename EV>
constexpr auto *bsr_kron_mfma_packed_kernel = &bsr_kron_mfma_form_kernel<true, NNZ, kpf, XL, EV>;

// complex<double>, 3x3 color blocks, 4x4 spin matrices with at most two nonzeros per row (the
// Wilson projectors 1 -+ gamma_mu, the identity, gamma matrices), from 8 rhs columns, spin first
// -- the reference's order (contract_kron_cols applies K_mu to x, then bsrmm the color blocks,
// bsr.h:933-998).  A lane owns one (block row, rhs column) pair and its 12 outputs, so no lane
// idles at any column count (pair p = row slot p / n, column p % n); per step (mu, d):
//   h(a) = c0 x(J_mu, d, col, b0) + c1 x(J_mu, d, col, b1)   (row a of K_mu as two terms: the
//                                                           host's table, build_kron_terms)
//   acc(i, a) += U_mu(i, d) h(a)
// i.e. 32 + 48 FMAs a step, no branches; the MFMA form spends 48 FMA-equivalents of 4x4x4 MFMA
// on the spin product of a dense K_mu and leaves a quarter of its lanes idle at 12 columns.
// Per wave and step one LDS-DMA group, one step ahead: x of the 64 pairs (4 KB: 16 pairs' 4
// spins a 1-KB piece, lane-linear over the pairs' 64-B spin runs, spin b of pair q at position
// b ^ (q / 4 % 4): a read of one spin by 16 lanes hits distinct banks in each of
// ds_read_b128's lane groups), U_mu(., d) of the wave's rows (<= 9 rows of 3 values, lanes <
// 32), and at d = 0 the wave rows' block columns of the next neighbour (one dword per row).
// Rows optionally visited in the host's XCD order (perm: each XCD's share of the row slots one
// compact lattice box).
constexpr int KS_WAVE_LDS = 2 * 4096 + 2 * 512 + 2 * 256;

/// The lane's pair in the spin-first kernels: wave w of XCD-contiguous workgroup wgi takes pairs
/// 64 (4 wgi + w) ... of the block_rows * n (row slot, column) pairs (launcher: below 2^31)
struct KronPair {
    int n, total;  ///< rhs columns, pairs
    int pw0;       ///< the wave's first pair
    int slot, col; ///< the lane's pair (past the end: the last one)
    bool live;     ///< ... and whether it has one
    /// false: the wave has no pair at all
    __device__ __forceinline__ bool init(const KronArgs &p, int lane, int w) {
        n = (int)p.ncols;
        total = (int)(p.block_rows * n);
        pw0 = (xcd_chunk(blockIdx.x, gridDim.x) * 4 + w) * 64;
        if (pw0 >= total) return false;
        const int pp = min(pw0 + lane, total - 1);
        live = pw0 + lane < total;
        slot = pp / n, col = pp - slot * n;
        return true;
    }
};

/// The accumulators of a step pinned: its products finish before what follows is issued (MEM:
/// and no memory access moves across)
template <bool MEM> __device__ __forceinline__ void pin_products(double (&ar)[3][4], double (&ai)[3][4]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if constexpr (MEM)
            asm volatile("" : "+v"(ar[i][0]), "+v"(ar[i][1]), "+v"(ar[i][2]), "+v"(ar[i][3]),
                         "+v"(ai[i][0]), "+v"(ai[i][1]), "+v"(ai[i][2]), "+v"(ai[i][3])::"memory");
        else
            asm volatile("" : "+v"(ar[i][0]), "+v"(ar[i][1]), "+v"(ar[i][2]), "+v"(ar[i][3]),
                         "+v"(ai[i][0]), "+v"(ai[i][1]), "+v"(ai[i][2]), "+v"(ai[i][3]));
}

__global__ void __launch_bounds__(256) bsr_kron_spin_kernel(const KronArgs p) {
    typedef double2 E;
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (launcher: pairs, x, values and block columns below 2^31 elements / bytes)
    KronPair pr;
    if (!pr.init(p, lane, w)) return;
    const int n = pr.n, nnz = p.nnz, total = pr.total, pw0 = pr.pw0;
    const int slot = pr.slot, col = pr.col;
    const bool live = pr.live;
    const int slot_lo = pw0 / n;
    const int rows_w = min(pw0 + 63, total - 1) / n - slot_lo + 1; // <= 9 (n >= 8)
    const int *perm = p.perm;
    auto row_of = [&](int slot) -> int { return perm ? perm[slot] : slot; };
    const int wr = slot - slot_lo;
    // LDS per wave: x slots [2][4096], U slots [2][512], J slots [2][256]
    char *wl = smem_s + w * KS_WAVE_LDS;
    const unsigned wl_a = lds_u32(wl);
    const E *xs = (const E *)wl;
    const E *us = (const E *)(wl + 8192);
    const int *js = (const int *)(wl + 9216);
    // x DMA: instruction k, lane l -> pair q = 16 k + l / 4, spin (l % 4) ^ (q / 4 % 4); its
    // (column * 4 + spin) in elements (-1: past the last pair) and wave row
    const int xd = 4 * n; // elements between the colors of a site
    int xcolb[4], xwr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = 16 * k + (lane >> 2);
        const int pq = pw0 + q, pc = min(pq, total - 1);
        const int b = (lane & 3) ^ ((q >> 2) & 3);
        const int sq = pc / n;
        xwr[k] = sq - slot_lo;
        xcolb[k] = pq < total ? (pc - sq * n) * 4 + b : -1;
    }
    // U DMA: lane l < 3 rows_w -> value i = l % 3 of wave row l / 3; J DMA: lane l < rows_w -> row l
    const bool u_ok = lane < 3 * rows_w;
    const int ui = lane % 3;
    const int ubase = (u_ok ? row_of(slot_lo + lane / 3) : 0) * nnz * 9 + (p.block_im_fast ? ui : 3 * ui);
    const int ustep = p.block_im_fast ? 3 : 1;
    const bool j_ok = lane < rows_w;
    const int jbase = (j_ok ? row_of(slot_lo + lane) : 0) * nnz;
    const int orow = row_of(slot); // the output row
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void *)p.x, (short)0, (int)(p.x_rows * 4 * n * 16), 0x00020000);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(
        (void *)p.v, (short)0, (int)(p.block_rows * nnz * 9 * 16), 0x00020000);
    const __amdgpu_buffer_rsrc_t rj = __builtin_amdgcn_make_buffer_rsrc(
        (void *)p.jj, (short)0, (int)(p.block_rows * nnz * 4), 0x00020000);
    // block columns of the x pieces for the current neighbour: mu = 0 from global memory, then
    // from the J slots
    int jx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) jx[k] = p.jj[row_of(slot_lo + xwr[k]) * nnz];
    // (offsets past the buffers for the pieces without data: the DMA writes zeros; selects, not
    // branches)
    unsigned xbad = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) xbad |= (xcolb[k] < 0 ? 1u : 0u) << k;
    const unsigned ubad = u_ok ? 0u : 0x80000000u, jbad = j_ok ? 0u : 0x80000000u;
    auto issue = [&](int mu, int d, int par) {
        const unsigned xb = wl_a + (unsigned)par * 4096u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned off = (unsigned)((jx[k] * 3 + d) * xd + xcolb[k]) * 16u;
            dma16(rx, (xbad >> k & 1) ? 0x80000000u : off, xb + (unsigned)k * 1024u);
        }
        if (lane < 32) dma16(ru, (unsigned)(ubase + mu * 9 + d * ustep) * 16u | ubad, wl_a + 8192u + (unsigned)par * 512u);
        if (d == 0 && mu + 1 < nnz)
            dma4(rj, (unsigned)(jbase + mu + 1) * 4u | jbad, wl_a + 9216u + (unsigned)((mu + 1) & 1) * 256u);
    };
    double ar[3][4], ai[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 4; ++a) ar[i][a] = 0, ai[i][a] = 0;
    // spin b of the lane's pair sits at piece 4 lane + (b ^ (lane / 4 % 4)) of an x slot: byte
    // address xa0 ^ 16 b
    const unsigned xa0 = (unsigned)(64 * lane + 16 * ((lane >> 2) & 3));
    const double *ctab = (const double *)p.ktab;          // [nnz][4 rows][2 terms] complex
    const int *btab = (const int *)(ctab + 16L * nnz);    // [nnz][4 rows][2 terms] spin index
    issue(0, 0, 0);
#pragma unroll 1
    for (int mu = 0; mu < nnz; ++mu) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int t = mu * 3 + d, par = t & 1;
            const bool more = t + 1 < 3 * nnz;
            // the slot about to be refilled was read in step t - 1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (more) {
                if (d == 2) {
                    // the next neighbour's block columns (landed with step t - 2's group)
#pragma unroll
                    for (int k = 0; k < 4; ++k) jx[k] = js[((mu + 1) & 1) * 64 + xwr[k]];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    issue(mu + 1, 0, par ^ 1);
                } else {
                    issue(mu, d + 1, par ^ 1);
                }
            }
            // step t's group landed; step t + 1's (5 instructions, 6 with a J piece) may stay in flight
            if (!more) wait_vmcnt(0);
            else if (d == 2 && mu + 2 < nnz) wait_vmcnt(6); // (mu + 1, 0) carries the J piece
            else wait_vmcnt(5);
            const char *xp = (const char *)(xs + par * 256);
            const E *up = us + par * 32 + wr * 3;
            E uv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) uv[i] = up[i];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                // (the compiler barrier keeps the scalar loads of the 12 rows of a neighbour from
                // being hoisted together: 96 SGPRs, spilled)
                asm volatile("" ::: "memory");
                // h(a) = c0 x(b0) + c1 x(b1): the row's (at most) two nonzero spin entries
                const int b0 = Uniform<int>::load(btab, mu * 8 + 2 * a);
                const int b1 = Uniform<int>::load(btab, mu * 8 + 2 * a + 1);
                const E x0 = *(const E *)(xp + (xa0 ^ (unsigned)(16 * b0)));
                const E x1 = *(const E *)(xp + (xa0 ^ (unsigned)(16 * b1)));
                const double c0r = Uniform<double>::load(ctab, mu * 16 + 4 * a);
                const double c0i = Uniform<double>::load(ctab, mu * 16 + 4 * a + 1);
                const double c1r = Uniform<double>::load(ctab, mu * 16 + 4 * a + 2);
                const double c1i = Uniform<double>::load(ctab, mu * 16 + 4 * a + 3);
                double hr = c0r * x0.x, hi = c0r * x0.y;
                hr = __builtin_fma(-c0i, x0.y, hr);
                hi = __builtin_fma(c0i, x0.x, hi);
                hr = __builtin_fma(c1r, x1.x, hr);
                hi = __builtin_fma(c1r, x1.y, hi);
                hr = __builtin_fma(-c1i, x1.y, hr);
                hi = __builtin_fma(c1i, x1.x, hi);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    ar[i][a] = __builtin_fma(uv[i].x, hr, ar[i][a]);
                    ar[i][a] = __builtin_fma(-uv[i].y, hi, ar[i][a]);
                    ai[i][a] = __builtin_fma(uv[i].x, hi, ai[i][a]);
                    ai[i][a] = __builtin_fma(uv[i].y, hr, ai[i][a]);
                }
            }
            // the step's products finish before the next step's waits and DMAs (otherwise the
            // compiler overlaps the steps and holds two steps' x values: 167 VGPRs)
            pin_products<false>(ar, ai);
        }
    }
    if (!live) return;
    store_outputs<E, 3, 4>((E *)p.y + ((long)orow * 3 * n + col) * 4, n, p.alpha_re, p.alpha_im, p.add,
                           [&](int i, int a) { return E{ar[i][a], ai[i][a]}; });
}


// The same spin-first product with the spin rows in "diagonal + XOR partner" form (every row a of
// K_mu nonzero at most at spins a and a ^ s_mu: the Wilson projectors 1 -+ gamma_mu and the gamma
// matrices in the chiral, Dirac-Pauli and DeGrand-Rossi bases), so that a lane keeps its pair's
// 4 spins in registers and the partner is a compile-time register (one instantiation of the
// step per s, chosen per neighbour by a scalar switch):
//   h(a) = c0(a) x(a) + c1(a) x(a ^ s)                  (the host's table, build_kron_terms)
//   acc(i, a) += U_mu(i, d) h(a)
// and everything comes by plain vector loads one step ahead (a pair's x: 64 contiguous bytes per
// lane and color; U_mu(., d) of its row; J_mu one neighbour ahead) -- no LDS and no LDS-DMA,
// whose issue cost (about 60 cycles a piece, MI355X_MICROARCH.md) set the first form's time.
/// h(a) = c0(a) x(a) + c1(a) x(a ^ S), the coefficients from the table by scalar loads
template <int S>
__device__ __forceinline__ void kron_xor_h(const double2 (&x)[4], const double *c, double (&hr)[4], double (&hi)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double c0r = Uniform<double>::load(c, 4 * a), c0i = Uniform<double>::load(c, 4 * a + 1);
        const double2 x0 = x[a], x1 = x[a ^ S];
        hr[a] = c0r * x0.x;
        hi[a] = c0r * x0.y;
        hr[a] = __builtin_fma(-c0i, x0.y, hr[a]);
        hi[a] = __builtin_fma(c0i, x0.x, hi[a]);
        if (S != 0) {
            const double c1r = Uniform<double>::load(c, 4 * a + 2), c1i = Uniform<double>::load(c, 4 * a + 3);
            hr[a] = __builtin_fma(c1r, x1.x, hr[a]);
            hi[a] = __builtin_fma(c1r, x1.y, hi[a]);
            hr[a] = __builtin_fma(-c1i, x1.y, hr[a]);
            hi[a] = __builtin_fma(c1i, x1.x, hi[a]);
        }
    }
}

__global__ void __launch_bounds__(256) bsr_kron_xor_kernel(const KronArgs p) {
    typedef double2 E;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (launcher: pairs, x and values below 2^31 elements)
    KronPair pr;
    if (!pr.init(p, lane, w)) return;
    const int n = pr.n, nnz = p.nnz, slot = pr.slot, col = pr.col;
    const bool live = pr.live;
    const int row = p.perm ? p.perm[slot] : slot;
    const E *x = (const E *)p.x, *v = (const E *)p.v;
    const int *jrow = p.jj + (long)row * nnz;
    const E *urow = v + (long)row * nnz * 9;
    const int xd = 4 * n; // elements between the colors of a site
    const int ust = p.block_im_fast ? 3 : 1, uis = p.block_im_fast ? 1 : 3;
    // the table: [nnz] { c[4 rows][c0 re, c0 im, c1 re, c1 im] } then [nnz] s
    const double *ctab = (const double *)p.ktab;
    const int *stab = (const int *)(ctab + 16L * nnz);
    double ar[3][4], ai[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 4; ++a) ar[i][a] = 0, ai[i][a] = 0;
    E xv[4], uv[3], xn[4], un[3];
    auto load = [&](int J, int mu, int d, E (&xo)[4], E (&uo)[3]) {
        const E *xp = x + (long)(J * 3 + d) * xd + col * 4;
#pragma unroll
        for (int b = 0; b < 4; ++b) xo[b] = xp[b];
        const E *up = urow + mu * 9 + d * ust;
#pragma unroll
        for (int i = 0; i < 3; ++i) uo[i] = up[i * uis];
    };
    int J = jrow[0];
    load(J, 0, 0, xv, uv);
#pragma unroll 1
    for (int mu = 0; mu < nnz; ++mu) {
        const int Jn = mu + 1 < nnz ? jrow[mu + 1] : J;
        const int sm = Uniform<int>::load(stab, mu);
        const double *c = ctab + mu * 16;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            // the next step's operands (the last step reloads its own: harmless)
            if (d < 2) load(J, mu, d + 1, xn, un);
            else load(Jn, mu + 1 < nnz ? mu + 1 : mu, 0, xn, un);
            // spin: one instantiation per partner (only h crosses the branches)
            double hr[4], hi[4];
            switch (sm) {
            case 0: kron_xor_h<0>(xv, c, hr, hi); break;
            case 1: kron_xor_h<1>(xv, c, hr, hi); break;
            case 2: kron_xor_h<2>(xv, c, hr, hi); break;
            default: kron_xor_h<3>(xv, c, hr, hi); break;
            }
            // color
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    ar[i][a] = __builtin_fma(uv[i].x, hr[a], ar[i][a]);
                    ar[i][a] = __builtin_fma(-uv[i].y, hi[a], ar[i][a]);
                    ai[i][a] = __builtin_fma(uv[i].x, hi[a], ai[i][a]);
                    ai[i][a] = __builtin_fma(uv[i].y, hr[a], ai[i][a]);
                }
            // the step's products finish before the next step's loads are issued
            pin_products<true>(ar, ai);
#pragma unroll
            for (int b = 0; b < 4; ++b) xv[b] = xn[b];
#pragma unroll
            for (int i = 0; i < 3; ++i) uv[i] = un[i];
        }
        J = Jn;
    }
    if (!live) return;
    store_outputs<E, 3, 4>((E *)p.y + ((long)row * 3 * n + col) * 4, n, p.alpha_re, p.alpha_im, p.add,
                           [&](int i, int a) { return E{ar[i][a], ai[i][a]}; });
}

// The adjoint, x with the image labels of A (the reference's local Kronecker operators throw
// "unsupported conjugation" there, bsr.h:399, 1032): for every domain site J of the component
//   y(J, d, n, b) = alpha * sum_{k : J(k) = J} sum_a conj(K_mu(a, b)) sum_i conj(U_k(i, d)) x(I, i, n, a)
// with k = I * nnz + mu A's nonzero index.  A site is pointed at by any number of nonzeros (halo
// sites by fewer; none at all is possible), so A^H is a row pointer over the sites and a list of
// k per site (bsr.cpp make_transposed), ascending: a fixed summation order.  The values are A's
// own arrays, block k and matrix mu read conj-transposed in place; no atomics; every offset
// into v, x and y is 64-bit.
struct KronAdjArgs {
    long sites; ///< A's domain sites of the component: the rows of A^H
    int nnz;    ///< A's nonzero blocks per block row (k = I * nnz + mu)
    int bi, bd, ki, kd; ///< A's block and Kronecker sizes (image, domain)
    const int *ptr; ///< [sites + 1] first entry of each site
    const int *ent; ///< A's nonzero index of each entry
    const void *v;
    const void *kron;
    int block_im_fast; ///< A's
    const void *x; ///< (A's block row, bi, ncols, ki)
    void *y;       ///< (site, bd, ncols, kd)
    long ncols;
    double alpha_re, alpha_im;
    int add;
};

/// Entries staged per pass of bsr_kron_adj_kernel, and the sites of a workgroup: 16 sites of a
/// 9-point stencil are 144 entries, one pass (a pass serves only the sites whose entries it
/// holds, the other lanes wait: with 128 entries for 21 sites of 12 columns every lane sat out
/// one of two passes, 373 us against 182 us for the forward product).  Staged from this many
/// columns (16^4 sites, staged / not, us: complex<double> n = 4 115 / 81, 12 253 / 220, 16 276 /
/// 266, 32 517 / 517, 64 957 / 979; complex<float> 4 73 / 58, 16 149 / 148, 32 296 / 308)
constexpr int KRON_ADJ_CHUNK = 160, KRON_ADJ_SITES = 16, KRON_ADJ_STAGE_COLS = 32;

/// A workgroup owns `S` consecutive sites x up to 256 columns (cpg columns per site), one thread
/// per (site, column) keeping its BD * KD outputs in registers.  STAGE (from KRON_ADJ_STAGE_COLS
/// columns): the workgroup's entries are one contiguous run of the entry list; their color blocks
/// are gathered into LDS conj-transposed, KRON_ADJ_CHUNK entries a pass (coalesced 16-byte pieces
/// of the 144-byte blocks, instead of every lane of a site fetching the same blocks through L1),
/// and read back as broadcasts.  With fewer columns too few lanes share a site for the pass and
/// its barriers to pay: each lane reads its blocks itself.  The spin matrices sit in LDS conj-transposed in both forms,
/// since the mu of an entry differs from site to site (a wave spanning several sites: no scalar
/// operand).  Per entry a lane reads the BI * KI x values of (I, ., column, .) -- consecutive
/// lanes consecutive columns, contiguous KI-element pieces -- one entry ahead, does the color
/// product t(d, a) = sum_i conj(U(i, d)) x(i, a), then the spin product
/// acc(d, b) += sum_a conj(K(a, b)) t(d, a), skipping the zeros of K.
/// Mixed (EV narrower than E, bsr.kron_mixed and bsr.kron_half): the conj-transposed images Us and Ks are widened
/// where they are staged, so the LDS layout and size are those of the same-type kernel of E and
/// the main loop is unchanged; a lane reading its blocks itself widens at the load.
template <typename EV, typename E, int BI, int BD, int KI, int KD, bool STAGE>
__global__ void __launch_bounds__(256) bsr_kron_adj_kernel(const KronAdjArgs p, int S, int cpg) {
    extern __shared__ __attribute__((aligned(16))) char smem_a[];
    constexpr int BLK = BI * BD, KK = KI * KD, CH = STAGE ? KRON_ADJ_CHUNK : 0;
    E *Us = (E *)smem_a; // [CH][BD][BI] conj(U(i, d))
    E *Ks = Us + CH * BLK; // [nnz][KD][KI] conj(K(a, b))
    const int nth = (int)blockDim.x;
    const EV *__restrict__ v = (const EV *)p.v;
    const EV *__restrict__ kron = (const EV *)p.kron;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const int tid = (int)threadIdx.x;
    const long r0 = (long)blockIdx.x * S;
    const int nrows = (int)std::min<long>(S, p.sites - r0);
    for (int e = tid; e < p.nnz * KK; e += nth) {
        const int mu = e / KK, w = e - mu * KK, b = w / KI, a = w - b * KI;
        Ks[e] = Ops<E>::conj(to_vec<E>(kron[(long)mu * KK + (p.block_im_fast ? a + b * KI : a * KD + b)]));
    }
    const int sl = tid / cpg;
    const long c = (long)blockIdx.y * cpg + tid % cpg;
    const bool live = sl < nrows && c < p.ncols;
    const long r = r0 + (live ? sl : 0);
    const int e0 = p.ptr[r0], e1 = p.ptr[r0 + nrows]; // the workgroup's entries
    const int lo = live ? p.ptr[r] : 0, hi = live ? p.ptr[r + 1] : 0; // the lane's
    const long xrow = p.ncols * KI;
    const E *xc = x + c * KI;
    E acc[BD][KD];
#pragma unroll
    for (int d = 0; d < BD; ++d)
#pragma unroll
        for (int b = 0; b < KD; ++b) acc[d][b] = Ops<E>::zero();
    auto load_x = [&](int k, E (&xo)[BI][KI]) {
        const E *xs = xc + (long)(k / p.nnz) * BI * xrow;
#pragma unroll
        for (int i = 0; i < BI; ++i)
#pragma unroll
            for (int a = 0; a < KI; ++a) xo[i][a] = xs[i * xrow + a];
    };
    if constexpr (!STAGE) __syncthreads(); // the spin matrices
    const int ustep = STAGE ? CH : std::max(e1 - e0, 1); // (not staged: one pass over the lane's entries)
    for (int base = e0; base < e1; base += ustep) {
        const int n = std::min(ustep, e1 - base);
        if constexpr (STAGE) {
            __syncthreads(); // the previous pass is consumed
            for (int t = tid; t < n * BLK; t += nth) {
                const int q = t / BLK, w = t - q * BLK, d = w / BI, i = w - d * BI;
                const long k = p.ent[base + q];
                Us[t] = Ops<E>::conj(to_vec<E>(v[k * BLK + (p.block_im_fast ? i + d * BI : i * BD + d)]));
            }
            __syncthreads();
        }
        const int a0 = std::max(lo, base), a1 = std::min(hi, base + n);
        if (a0 >= a1) continue;
        int k = p.ent[a0];
        E xa[BI][KI];
        load_x(k, xa);
#pragma unroll 1
        for (int e = a0; e < a1; ++e) {
            const int mu = k % p.nnz;
            E ug[BD][BI]; // not staged: the lane's own copy of the block
            if constexpr (!STAGE) {
                const EV *ub = v + (long)k * BLK;
#pragma unroll
                for (int d = 0; d < BD; ++d)
#pragma unroll
                    for (int i = 0; i < BI; ++i)
                        ug[d][i] = Ops<E>::conj(to_vec<E>(ub[p.block_im_fast ? i + d * BI : i * BD + d]));
            }
            E xb[BI][KI];
            if (e + 1 < a1) {
                k = p.ent[e + 1];
                load_x(k, xb);
            }
            const E *U = Us + (e - base) * BLK;
            const E *K = Ks + mu * KK;
            // color: t(d, a) = sum_i conj(U(i, d)) x(i, a)
            E t[BD][KI];
#pragma unroll
            for (int d = 0; d < BD; ++d)
#pragma unroll
                for (int a = 0; a < KI; ++a) t[d][a] = Ops<E>::zero();
#pragma unroll
            for (int i = 0; i < BI; ++i)
#pragma unroll
                for (int d = 0; d < BD; ++d) {
                    const E u = STAGE ? U[d * BI + i] : ug[d][i];
#pragma unroll
                    for (int a = 0; a < KI; ++a) t[d][a] = Ops<E>::fma(u, xa[i][a], t[d][a]);
                }
            // spin: acc(d, b) += sum_a conj(K(a, b)) t(d, a)
#pragma unroll
            for (int b = 0; b < KD; ++b)
#pragma unroll
                for (int a = 0; a < KI; ++a) {
                    const E kk = K[b * KI + a];
                    if (!Ops<E>::nonzero(kk)) continue;
#pragma unroll
                    for (int d = 0; d < BD; ++d) acc[d][b] = Ops<E>::fma(kk, t[d][a], acc[d][b]);
                }
            if (e + 1 < a1) {
#pragma unroll
                for (int i = 0; i < BI; ++i)
#pragma unroll
                    for (int a = 0; a < KI; ++a) xa[i][a] = xb[i][a];
            }
        }
    }
    if (!live) return;
    store_outputs<E, BD, KD>(y + (r * BD * p.ncols + c) * KD, p.ncols, p.alpha_re, p.alpha_im, p.add,
                             [&](int d, int b) { return acc[d][b]; });
}

/// Any block / Kronecker sizes: one thread per output element (site, d, column, b)
template <typename EV, typename E>
__global__ void __launch_bounds__(256) bsr_kron_adj_generic_kernel(const KronAdjArgs p) {
    const EV *__restrict__ v = (const EV *)p.v;
    const EV *__restrict__ kron = (const EV *)p.kron;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const long total = p.sites * p.bd * p.ncols * p.kd;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
        const int b = (int)(idx % p.kd);
        long t = idx / p.kd;
        const long c = t % p.ncols;
        t /= p.ncols;
        const int d = (int)(t % p.bd);
        const long r = t / p.bd;
        E acc = Ops<E>::zero();
        for (int e = p.ptr[r]; e < p.ptr[r + 1]; ++e) {
            const long k = p.ent[e];
            const long I = k / p.nnz, mu = k - I * p.nnz;
            const E *xs = x + (I * p.bi * p.ncols + c) * p.ki;
            const EV *K = kron + mu * p.ki * p.kd;
            const EV *U = v + k * p.bi * p.bd;
            for (int a = 0; a < p.ki; ++a) {
                const E kk = to_vec<E>(p.block_im_fast ? K[a + b * p.ki] : K[a * p.kd + b]);
                if (!Ops<E>::nonzero(kk)) continue;
                E s = Ops<E>::zero();
                for (int i = 0; i < p.bi; ++i) {
                    const E u = to_vec<E>(p.block_im_fast ? U[i + d * p.bi] : U[i * p.bd + d]);
                    s = Ops<E>::fma(Ops<E>::conj(u), xs[i * p.ncols * p.ki + a], s);
                }
                acc = Ops<E>::fma(Ops<E>::conj(kk), s, acc);
            }
        }
        E o = Ops<E>::scale(acc, p.alpha_re, p.alpha_im);
        if (p.add) o = Ops<E>::add(o, y[idx]);
        y[idx] = o;
    }
}

constexpr long KRON_LDS_BYTES = 64 * 1024;

/// 3x3 color blocks and 4x4 spin matrices: the sizes of the specialised kernels
template <typename Args> bool is_3x3_4x4(const Args &a) { return a.bi == 3 && a.bd == 3 && a.ki == 4 && a.kd == 4; }

/// The matrix-core kernels' XL: neighbours of x staged ahead by LDS-DMA ("bsr.kron_xlds", 0-3); 0
/// where x or y reach beyond the DMA's 32-bit buffer offsets
int kron_xl(const KronArgs &a) {
    const bool fits = std::max(a.block_rows * 12L, a.x_rows * 4L) * a.ncols * 16 < (1L << 31);
    return fits ? std::max(0, std::min(3, g_bsr_tune.kron_xlds)) : 0;
}

/// f(EV{}, E{}) with EV the values' type and E the vectors': the same type, single-precision
/// values under double vectors, or half-precision values under single vectors
template <typename F> void with_kron_types(const BsrDesc &d, F f) {
    if (d.tv == d.t) switch (d.t) {
        case SBX_CDOUBLE: return f(double2{}, double2{});
        case SBX_CFLOAT: return f(float2{}, float2{});
        case SBX_DOUBLE: return f(double{}, double{});
        case SBX_FLOAT: return f(float{}, float{});
        default: break;
        }
    if (d.tv == SBX_CFLOAT && d.t == SBX_CDOUBLE) return f(float2{}, double2{});
    if (d.tv == SBX_FLOAT && d.t == SBX_DOUBLE) return f(float{}, double{});
    if (d.tv == SBX_CHALF && d.t == SBX_CFLOAT) return f(f16x2{}, float2{});
    if (d.tv == SBX_HALF && d.t == SBX_FLOAT) return f(f16{}, float{});
    throw Error("kron bsr: unsupported type");
}

/// EV: the values' type, E: the vectors' (EV = E, float / float2 under double / double2, or
/// f16 / f16x2 under float / float2)
template <typename EV, typename E> void launch_kron_adj_typed(const KronAdjArgs &a, hipStream_t s) {
    KernelTimer timer("bsr", s);
    if (g_bsr_tune.kron_adj && is_3x3_4x4(a)) {
        const int cpg = (int)std::min<long>(a.ncols, 256);
        const bool stage = a.ncols >= KRON_ADJ_STAGE_COLS && g_bsr_tune.kron_adj != 2;
        const int S = std::min(256 / cpg, stage ? KRON_ADJ_SITES : 256);
        const int nth = (S * cpg + 63) / 64 * 64; // whole waves, at most 256 threads
        const long gx = (a.sites + S - 1) / S, gy = (a.ncols + cpg - 1) / cpg;
        // (the LDS images are in the vectors' type: a mixed launch widens them at the staging)
        const long lds = (long)((stage ? KRON_ADJ_CHUNK * 9 : 0) + (long)a.nnz * 16) * (long)sizeof(E);
        if (lds <= KRON_LDS_BYTES && gx < (1L << 31) && gy < 65536) {
            g_bsr_tune.last = 15;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(nth), (size_t)lds, s, a, S, cpg);
            };
            if (stage) go(bsr_kron_adj_kernel<EV, E, 3, 3, 4, 4, true>);
            else go(bsr_kron_adj_kernel<EV, E, 3, 3, 4, 4, false>);
            SBX_HIP_CHECK(hipGetLastError());
            return;
        }
    }
    // (16 with last_mixed 1 already means bsr_blk_mfma_kernel's mixed form: the mixed launch here is 19)
    g_bsr_tune.last = std::is_same<EV, E>::value ? 16 : 19;
    const long total = a.sites * a.bd * a.ncols * a.kd;
    const long blocks = std::min((total + 255) / 256, 65536L);
    hipLaunchKernelGGL((bsr_kron_adj_generic_kernel<EV, E>), dim3(blocks), dim3(256), 0, s, a);
    SBX_HIP_CHECK(hipGetLastError());
}

/// The adjoint of a Kronecker operator: the descriptor speaks of A^H (BsrDesc), the kernels of A
void launch_bsr_kron_adj(const BsrDesc &d, int device) {
    if (d.num_nnz_per_row <= 0 || !d.kron || !d.adj_ent || !d.x_row_major || !d.y_row_major)
        throw Error("kron bsr: internal error (adjoint layout or pattern)");
    set_device(device);
    g_bsr_tune.last = 0;
    KronAdjArgs a{};
    a.sites = d.block_rows;
    a.nnz = d.num_nnz_per_row;
    a.bi = d.bd;
    a.bd = d.bi;
    a.ki = d.kd;
    a.kd = d.ki;
    a.ptr = d.adj_ptr;
    a.ent = d.adj_ent;
    a.v = d.v;
    a.kron = d.kron;
    a.block_im_fast = d.block_im_fast ? 0 : 1;
    a.x = d.x;
    a.y = d.y;
    a.ncols = d.ncols;
    a.alpha_re = d.alpha.re;
    a.alpha_im = d.alpha.im;
    a.add = d.add ? 1 : 0;
    hipStream_t s = get_stream(device);
    with_kron_types(d, [&](auto ev, auto e) { launch_kron_adj_typed<decltype(ev), decltype(e)>(a, s); });
}

/// EV: the values' type, E: the vectors' (EV = E, float / float2 under double / double2, or
/// f16 / f16x2 under float / float2)
template <typename EV, typename E> void launch_kron_typed(const KronArgs &a, hipStream_t s) {
    KernelTimer timer("bsr", s);
    constexpr bool same = std::is_same<EV, E>::value;
    // (bsr_kron_lds_kernel's LDS image holds the values as stored, padded to whole dwords, then
    // the block columns)
    auto lds_rows = [&](long S) {
        return kron_lds_values_bytes<EV>(S * a.nnz * a.bi * a.bd) + S * a.nnz * (long)sizeof(int);
    };
    // the spin-first kernels read their tables of doubles: same-type products only
    if constexpr (std::is_same<E, double2>::value && same) {
        if (g_bsr_tune.kron_spin == 2 && a.xtab && is_3x3_4x4(a) && a.nnz >= 1 &&
            a.ncols >= g_bsr_tune.kron_spin_min_cols && a.x_rows * 4 * a.ncols < (1L << 31) &&
            a.block_rows * a.ncols + 1024 < (1L << 31)) {
            const long waves = (a.block_rows * a.ncols + 63) / 64, blocks = (waves + 3) / 4;
            if (blocks < (1L << 31)) {
                g_bsr_tune.last = 12;
                KronArgs b = a;
                b.ktab = a.xtab;
                hipLaunchKernelGGL(bsr_kron_xor_kernel, dim3((unsigned)blocks), dim3(256), 0, s, b);
                SBX_HIP_CHECK(hipGetLastError());
                return;
            }
        }
        if (g_bsr_tune.kron_spin == 1 && a.ktab && is_3x3_4x4(a) && a.nnz >= 1 && a.nnz <= 64 &&
            a.ncols >= std::max(8L, g_bsr_tune.kron_spin_min_cols) &&
            a.block_rows * a.nnz * 9 * 16 < (1L << 31) && a.x_rows * 4 * a.ncols * 16 < (1L << 31) &&
            a.block_rows * a.ncols + 1024 < (1L << 31)) {
            const long waves = (a.block_rows * a.ncols + 63) / 64, blocks = (waves + 3) / 4;
            if (blocks < (1L << 31)) {
                g_bsr_tune.last = 9;
                const size_t lds = 4 * (size_t)KS_WAVE_LDS;
                hipLaunchKernelGGL(bsr_kron_spin_kernel, dim3((unsigned)blocks), dim3(256), lds, s, a);
                SBX_HIP_CHECK(hipGetLastError());
                return;
            }
        }
    }
    if constexpr (std::is_same<E, double2>::value) {
        // complex<float> values (bsr.kron_mixed) take the same conditions and the same column
        // bound, kron_mfma_min_cols (8), as complex<double> ones.  Measured against the mixed VALU
        // form (bsr_kron_lds_kernel<float2, double2>; tools/studies/kron_mixed.py,
        // profiles/kron_mixed_measure.txt, 16^4 and 16^3 x 64): the matrix-core forms are 1.35-1.9x
        // faster at 8, 12, 16, 32 and 64 columns, the round-to-round spreads below 2 % of either
        // time -- so from 8 columns they are taken.  They were faster at 1 and 4 columns too
        // (1.2x, 2.0x: kron_mfma_min_cols 1 takes them there); the default bound is not lowered
        // for one pair of types alone, and 2, 3 and 5-7 columns (5 and 7 do not pack) are not
        // measured.
        // (the 2 GiB bound: the colour run's LDS-DMA buffer offsets; the mixed form stages the run
        // by plain loads with 64-bit addresses)
        if (g_bsr_tune.kron_mfma && is_3x3_4x4(a) && a.nnz == 9 &&
            a.ncols >= g_bsr_tune.kron_mfma_min_cols && (!same || a.block_rows * 81L * 16 < (1L << 31))) {
            // packed slots: W waves of 16 (row, column) slots hold RW = 16 W / n whole rows
            int wpk = 0;
            for (int wv = 4; wv >= 1 && g_bsr_tune.kron_pack; --wv)
                if (a.ncols < 16 && (16 * wv) % a.ncols == 0 && 16 * wv / a.ncols <= 32) {
                    wpk = wv;
                    break;
                }
            if (wpk > 0) {
                const int rw = (int)(16 * wpk / a.ncols);
                const long blocks = (a.block_rows + rw - 1) / rw;
                if (blocks < (1L << 31)) {
                    g_bsr_tune.last = 6;
                    // LDS: rw rows of 81 color values, rounded up to whole DMA passes of the
                    // workgroup (the lanes past the run write zeros)
                    const int nth = 64 * wpk;
                    // (mixed: the same count of 8-byte values, a multiple of 16 bytes as nth is of 64;
                    // staged by plain loads bounded by the run: no DMA pass to size for)
                    const size_t lds_cb = (size_t)((rw * 81 + nth - 1) / nth * nth) * sizeof(EV);
                    // the DMA loop: passes u < ceil(nrows * 81 / nth), nrows <= rw
                    if (same) check_dma_lds("bsr_kron_mfma_packed_kernel", lds_cb, (rw * 81L + nth - 1) / nth, nth);
                    // x by LDS-DMA: a ring of 2 x 3 KB per wave after the color blocks (lds_cb is
                    // a multiple of 16); 32-bit buffer offsets
                    const int xl = kron_xl(a);
                    // (+ the 9 spin matrices)
                    const size_t lds_bytes = lds_cb + (xl > 0 ? (size_t)wpk * (xl + 1) * 3072 + 9 * 16 * 16 : 0);
                    if (xl) check_dma_lds("bsr_kron_mfma_packed_kernel x ring", lds_bytes, 0, 0, (long)lds_cb + wpk * (xl + 1) * 3072L + 9 * 16 * 16);
                    // spin matrices one neighbour ahead: n = 8 / 12 104 / 166 -> 102 / 163 us
                    // (the one-row-per-wave kernel: 214 -> 221 us at n = 16, so not there;
                    // profiles/r02c_kron_kpf.txt)
                    auto go = [&](auto kern) {
                        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * wpk), lds_bytes, s, a, rw, (int)lds_cb);
                    };
                    if (xl == 1) go(bsr_kron_mfma_packed_kernel<9, true, 1, EV>);
                    else if (xl == 2) go(bsr_kron_mfma_packed_kernel<9, true, 2, EV>);
                    else if (xl == 3) go(bsr_kron_mfma_packed_kernel<9, true, 3, EV>);
                    else go(bsr_kron_mfma_packed_kernel<9, true, 0, EV>);
                    SBX_HIP_CHECK(hipGetLastError());
                    return;
                }
            }
            const long ngroups = (a.ncols + 15) / 16;
            const long tasks = a.block_rows * ngroups, blocks = (tasks + 3) / 4;
            if (blocks < (1L << 31)) {
                g_bsr_tune.last = 5;
                // x by LDS-DMA (32-bit buffer offsets)
                const int xl = kron_xl(a);
                auto go = [&](auto kern) {
                    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, a, (int)ngroups, 0);
                };
                if (xl == 1) go(bsr_kron_mfma_kernel<9, false, 1, EV>);
                else if (xl == 2) go(bsr_kron_mfma_kernel<9, false, 2, EV>);
                else if (xl == 3) go(bsr_kron_mfma_kernel<9, false, 3, EV>);
                else go(bsr_kron_mfma_kernel<9, false, 0, EV>);
                SBX_HIP_CHECK(hipGetLastError());
                return;
            }
        }
    }
    if (is_3x3_4x4(a) && a.nnz == 9 && a.ncols >= 4 &&
        lds_rows(256 / std::min<long>(a.ncols, 256)) <= KRON_LDS_BYTES) {
        const int cpg = (int)std::min<long>(a.ncols, 256);
        const int S = 256 / cpg;
        const dim3 grid((unsigned)((a.block_rows + S - 1) / S), (unsigned)((a.ncols + cpg - 1) / cpg));
        hipLaunchKernelGGL((bsr_kron_lds_kernel<EV, E, 3, 3, 4, 4, 9>), grid, dim3(256),
                           (size_t)lds_rows(S), s, a, S, cpg);
    } else if (is_3x3_4x4(a)) {
        const long total = a.block_rows * a.ncols;
        const long blocks = std::min((total + 255) / 256, 65536L);
        hipLaunchKernelGGL((bsr_kron_kernel<EV, E, 3, 3, 4, 4>), dim3(blocks), dim3(256), 0, s, a);
    } else {
        const long total = a.block_rows * a.bi * a.ncols * a.ki;
        const long blocks = std::min((total + 255) / 256, 65536L);
        hipLaunchKernelGGL((bsr_kron_generic_kernel<EV, E>), dim3(blocks), dim3(256), 0, s, a);
    }
    SBX_HIP_CHECK(hipGetLastError());
}

} // namespace

void launch_bsr_kron(const BsrDesc &d, int device) {
    if (d.block_rows == 0 || d.ncols == 0) return;
    if (d.adj_ptr) return launch_bsr_kron_adj(d, device);
    if (d.num_nnz_per_row <= 0 || !d.kron || !d.x_row_major || !d.y_row_major)
        throw Error("kron bsr: internal error (layout or pattern)");
    set_device(device);
    g_bsr_tune.last = 0;
    hipStream_t s = get_stream(device);
    KronArgs a{};
    a.block_rows = d.block_rows;
    a.nnz = d.num_nnz_per_row;
    a.bi = d.bi;
    a.bd = d.bd;
    a.ki = d.ki;
    a.kd = d.kd;
    a.jj = d.jj;
    a.v = d.v;
    a.kron = d.kron;
    a.block_im_fast = d.block_im_fast ? 1 : 0;
    a.x = d.x;
    a.y = d.y;
    a.ncols = d.ncols;
    a.alpha_re = d.alpha.re;
    a.alpha_im = d.alpha.im;
    a.add = d.add ? 1 : 0;
    a.ylds = g_bsr_tune.kron_ylds ? 1 : 0;
    // domain sites can exceed block_rows (halo sites): the x staging's 32-bit buffer offsets are
    // bounded by x's extent, not y's
    a.x_rows = d.x_rows > 0 ? d.x_rows : d.block_rows * d.bd;
    a.perm = g_bsr_tune.kron_order ? d.kron_perm : nullptr;
    // (the spin-first tables: null on a mixed launch, whose operator never builds them)
    a.ktab = d.tv == d.t ? d.kron_terms : nullptr;
    a.xtab = d.tv == d.t ? d.kron_xor : nullptr;
    with_kron_types(d, [&](auto ev, auto e) { launch_kron_typed<decltype(ev), decltype(e)>(a, s); });
}

} // namespace sbx
