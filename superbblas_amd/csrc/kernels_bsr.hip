// Block-sparse (BSR) matrix times dense tensor -- the `bsr_krylov` hot loop.
//
// Reference: BSR<Cpu>::operator() builtin loop (bsr.h:535-650; one small GEMM/GEMV per nonzero
// block, OpenMP over block rows) and BSR<Gpu> -> hipsparseXbsrmm (bsr.h:855-928).
// Here: one thread per output element y(row-block i, image component c, rhs column n).
//  * The thread order follows the output layout so the stores are coalesced: for a row-major
//    output (rhs fastest) consecutive lanes take consecutive rhs columns, the nonzero block
//    values are then wave-uniform (broadcast loads) and the x gathers are contiguous along the
//    rhs; for a column-major output consecutive lanes take consecutive image components/rows
//    and read consecutive 16-byte pieces of the row-ordered nonzero blocks.
//  * Bound: HBM (the nonzero blocks are streamed once; x is re-read through L2/MALL).
//  * ELL operators (every block row has the same number of nonzero blocks -- the lattice
//    stencils) use bsr_ell_kernel: a workgroup streams the nonzero blocks of a chunk of block
//    rows into LDS with coalesced 16-byte loads (the value stream is the dominant HBM traffic),
//    then every thread computes all `bi` outputs of one (block row, rhs column) pair reading the
//    blocks from LDS (broadcast across the rhs lanes) and x from global memory (contiguous along
//    the rhs for row-major x).
#include "elem_ops.h"
#include "kernel_util.h"
#include "sbx_internal.h"

#include <algorithm>
#include <type_traits>

namespace sbx {
BsrTune g_bsr_tune;
namespace {

struct BsrArgs {
    long block_rows;
    int bi, bd;
    const int *ii;
    const int *jj;
    const void *v;
    int block_im_fast;
    const void *x;
    long ldx;
    long x_rows; // domain rows of x
    void *y;
    long ldy;
    long ncols;
    double alpha_re, alpha_im;
    int add;
    int ilv = 1; // bsr_ell9_kernel: an XCD's chunks visited as ilv interleaved parts
    int nt = 0;  // the value stream's LDS-DMA loads non-temporal: g_bsr_tune.nt's kernel bits
    // site tiles (bsr_ell9_tile_kernel; [0] 16-site, [1] 8-site tiles; rows == nullptr: none)
    TileSched tiles[2];
};

// (widen / to_vec, a value of the operator's type as the vectors' type: elem_ops.h)

// The generic form, any block size, pattern and layout: one thread per output element, for
//  * same-type products (EV == EX; BI_, BD_ > 0: a compile-time block shape);
//  * mixed products: an operator kept in single precision (EV: float, float2) applied to vectors
//    of the double counterpart (EX), or one kept in half precision (EV: f16, f16x2) applied to
//    vectors of the single counterpart.  The values are read in place as EV and widened at the
//    load (exact); products, sums, alpha and the store of y are in EX's precision.  No converted
//    copy of the values exists;
//  * ADJ, the in-place adjoint (bsr.adj_inplace): the transposed pattern with an entry
//    indirection.  The output element is (block column J of A, component c, rhs column); entry j
//    of J reads block ent[j] of A's own value array -- the same storage as the copy's block j,
//    p.block_im_fast being the opposite of A's -- conjugated (and widened, both exact) at the
//    load.  Entries in list order (ascending nonzero index of A: the copy's order): the bits of
//    the forward form on the conjugated copy.  A block column with no entry writes alpha * 0
//    (plus y when adding).
// Every form takes a row's entries in order and the bd elements ascending with Ops<EX>::fma, so
// the result is the same from run to run.  Offsets into v, x and y are 64-bit (the forward
// forms' element offset inside a block is an int below bi * bd).
template <typename EV, typename EX, int BI_, int BD_, bool YROW, bool XROW, bool ADJ>
__global__ void __launch_bounds__(256) bsr_kernel(const BsrArgs p, const int *__restrict__ ent) {
    const int bi = BI_ > 0 ? BI_ : p.bi;
    const int bd = BD_ > 0 ? BD_ : p.bd;
    const long total = p.block_rows * bi * p.ncols;
    const EV *__restrict__ v = (const EV *)p.v;
    const EX *__restrict__ x = (const EX *)p.x;
    EX *__restrict__ y = (EX *)p.y;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
        long i, col;
        int c;
        if (YROW) {
            col = idx % p.ncols;
            const long t = idx / p.ncols;
            c = (int)(t % bi);
            i = t / bi;
        } else {
            c = (int)(idx % bi);
            const long t = idx / bi;
            i = t % p.block_rows;
            col = t / p.block_rows;
        }
        EX acc = Ops<EX>::zero();
        const int j0 = p.ii[i], j1 = p.ii[i + 1];
        for (int j = j0; j < j1; ++j) {
            // The adjoint keeps the 64-bit index arithmetic and the loop without a skip test that
            // it was measured with (the transposed pattern holds no skipped block): with the
            // forward form's int indices and its test -- a branch on d0 ahead of the load of
            // ent[j] -- form 18 was 6-17 % slower (profiles/bsr_kernels_refactor_measure.txt)
            typedef typename std::conditional<ADJ, long, int>::type K;
            const K d0 = p.jj[j];
            if (!ADJ && d0 < 0) continue;
            const EV *vb = v + (long)(ADJ ? ent[j] : j) * bi * bd;
            for (int e = 0; e < bd; ++e) { // (BD_ > 0: a compile-time trip count)
                EV a = p.block_im_fast ? vb[c + (K)e * bi] : vb[(K)c * bd + e];
                if constexpr (ADJ) a = Ops<EV>::conj(a);
                const EX xv = XROW ? x[(long)(d0 + e) * p.ldx + col] : x[(d0 + e) + col * p.ldx];
                acc = Ops<EX>::fma(to_vec<EX>(a), xv, acc);
            }
        }
        const long img = i * bi + c;
        EX *yp = YROW ? y + img * p.ldy + col : y + img + col * p.ldy;
        const EX out = Ops<EX>::scale(acc, p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<EX>::add(*yp, out) : out;
    }
}

/// The generic form's launch: the kernel of the two layouts
template <typename EV, typename EX, int BI, int BD, bool ADJ = false>
void launch_generic(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s, const int *ent = nullptr) {
    const long total = a.block_rows * a.bi * a.ncols;
    const long blocks = std::min((total + 255) / 256, 65536L);
    KernelTimer timer("bsr", s);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a, ent); };
    if (yrow && xrow) go(bsr_kernel<EV, EX, BI, BD, true, true, ADJ>);
    else if (yrow) go(bsr_kernel<EV, EX, BI, BD, true, false, ADJ>);
    else if (xrow) go(bsr_kernel<EV, EX, BI, BD, false, true, ADJ>);
    else go(bsr_kernel<EV, EX, BI, BD, false, false, ADJ>);
    SBX_HIP_CHECK(hipGetLastError());
}

constexpr int ELL_LDS_BYTES = 24576; // per workgroup: several workgroups share a CU

template <typename E, int BI, int BD, int G, bool YROW, bool XROW>
__global__ void __launch_bounds__(256) bsr_ell_kernel(const BsrArgs p, int nnz, int rb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BLK = BI * BD;
    E *vals = (E *)smem;
    int *cols = (int *)(smem + (size_t)rb * nnz * BLK * sizeof(E));
    const E *__restrict__ v = (const E *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    // consecutive chunks of block rows on one XCD: neighbouring sites share x rows in its L2
    const int chunk = xcd_chunk(blockIdx.x, gridDim.x);
    const long row0 = (long)chunk * rb;
    const int nrows = (int)min((long)rb, p.block_rows - row0);
    // 1) stream the chunk's nonzero blocks (contiguous in the ELL value array) and block
    //    columns into LDS, 8 loads in flight per thread
    const long vbase = row0 * nnz * BLK;
    const int nv = nrows * nnz * BLK;
    for (int e0 = threadIdx.x; e0 < nv; e0 += 256 * 8) {
        E t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = v[vbase + min(e0 + 256 * q, nv - 1)];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (e0 + 256 * q < nv) vals[e0 + 256 * q] = t[q];
    }
    for (int e = threadIdx.x; e < nrows * nnz; e += 256) cols[e] = p.jj[row0 * nnz + e];
    __syncthreads();
    // 2) every thread computes the BI x G outputs of a (block row, group of G rhs columns); the
    //    x rows of block j+1 are fetched while block j is applied
    const long ngroups = (p.ncols + G - 1) / G;
    const long npairs = (long)nrows * ngroups;
    for (long q = threadIdx.x; q < npairs; q += 256) {
        int r;
        long g;
        if (YROW) {
            r = (int)(q / ngroups);
            g = q % ngroups;
        } else {
            r = (int)(q % nrows);
            g = q / nrows;
        }
        long colv[G];
#pragma unroll
        for (int k = 0; k < G; ++k) colv[k] = min(g * G + k, p.ncols - 1);
        E acc[BI][G];
#pragma unroll
        for (int c = 0; c < BI; ++c)
#pragma unroll
            for (int k = 0; k < G; ++k) acc[c][k] = Ops<E>::zero();
        const int *jr = cols + r * nnz;
        const E *vr = vals + r * nnz * BLK;
        auto fetch = [&](int d0, E (*xv)[G]) {
            const long d = d0 < 0 ? 0 : d0;
#pragma unroll
            for (int e = 0; e < BD; ++e)
#pragma unroll
                for (int k = 0; k < G; ++k)
                    xv[e][k] = XROW ? x[(d + e) * p.ldx + colv[k]] : x[(d + e) + colv[k] * p.ldx];
        };
        E xn[BD][G];
        int dn = jr[0];
        fetch(dn, xn);
        for (int j = 0; j < nnz; ++j) {
            E xc[BD][G];
#pragma unroll
            for (int e = 0; e < BD; ++e)
#pragma unroll
                for (int k = 0; k < G; ++k) xc[e][k] = xn[e][k];
            const int dc = dn;
            if (j + 1 < nnz) {
                dn = jr[j + 1];
                fetch(dn, xn);
            }
            if (dc < 0) continue;
            const E *vb = vr + j * BLK;
#pragma unroll
            for (int e = 0; e < BD; ++e)
#pragma unroll
                for (int c = 0; c < BI; ++c) {
                    const E a = p.block_im_fast ? vb[c + e * BI] : vb[c * BD + e];
#pragma unroll
                    for (int k = 0; k < G; ++k) acc[c][k] = Ops<E>::fma(a, xc[e][k], acc[c][k]);
                }
        }
#pragma unroll
        for (int c = 0; c < BI; ++c) {
            const long img = (row0 + r) * BI + c;
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const long col = g * G + k;
                if (col >= p.ncols) break;
                E *yp = YROW ? y + img * p.ldy + col : y + img + col * p.ldy;
                const E out = Ops<E>::scale(acc[c][k], p.alpha_re, p.alpha_im);
                *yp = p.add ? Ops<E>::add(*yp, out) : out;
            }
        }
    }
}

// Large blocks (12x12 spin x color, the Wilson-like operator): block-row products on the FP64
// (FP32) matrix cores.  A wave owns one block row and a tile of 16 rhs columns and computes the
// 16x16 tile  Y_i = sum_j A_ij X_j  with v_mfma_f64_16x16x4_f64 or v_mfma_f32_16x16x4f32 (tile
// rows >= BI are padding), K running over the BD domain rows of every nonzero block (BD/4 steps
// per block, 4 real MFMAs per complex step).  The generic kernels read the fragments straight
// from global memory: lane l reads A_ij[l&15][k+(l>>4)] and x[d_j+k+(l>>4)][col0+(l&15)]
// (contiguous along the rhs for row-major x); out-of-range rows, columns and skipped blocks
// (-1 columns) are clamped loads replaced by zero, so the loop has no divergent branches.
// (BsrNarrow / BsrStored, an element of a narrower operator as it lies in memory: elem_ops.h)

template <typename R, bool CPLX> struct BsrMfmaElem;
template <> struct BsrMfmaElem<double, true> { typedef double2 type; };
template <> struct BsrMfmaElem<double, false> { typedef double type; };
template <> struct BsrMfmaElem<float, true> { typedef float2 type; };
template <> struct BsrMfmaElem<float, false> { typedef float type; };
template <> struct BsrMfmaElem<f16, true> { typedef f16x2 type; }; // (operator values only)
template <> struct BsrMfmaElem<f16, false> { typedef f16 type; };
// BsrMfmaElem's inverse: the real type and the complexity of an element type
template <typename E> struct BsrMfmaScalar { typedef E real; static constexpr bool cplx = false; };
template <> struct BsrMfmaScalar<double2> { typedef double real; static constexpr bool cplx = true; };
template <> struct BsrMfmaScalar<float2> { typedef float real; static constexpr bool cplx = true; };
template <> struct BsrMfmaScalar<f16x2> { typedef f16 real; static constexpr bool cplx = true; };
// 16x16x4 MFMA per real type and its C/D row map (col = lane & 15)
template <typename R> struct BsrMfma;
template <> struct BsrMfma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int q) { return (lane >> 4) + 4 * q; }
};
template <> struct BsrMfma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int q) { return 4 * (lane >> 4) + q; }
};

// One block row per wave, the fragments of nonzero block t+1 loaded while block t is applied
// (twice the bytes in flight per wave; 985 -> 880 us on the chain's complex<float> operator).
// Mapping consecutive block rows to one XCD was measured no faster.
template <typename RV, typename R, bool CPLX, int BI, int BD, bool YROW, bool XROW>
__global__ void __launch_bounds__(256) bsr_mfma_pf_kernel(const BsrArgs p, long ntiles_n) {
    typedef typename BsrMfmaElem<R, CPLX>::type E; // the vectors; the values as stored, widening at the load:
    typedef typename BsrStored<typename BsrMfmaElem<RV, CPLX>::type, E>::type EV;
    typedef typename BsrMfma<R>::acc_t acc_t;
    static_assert(BI <= 16 && BD % 4 == 0, "block shape");
    constexpr int KS = BD / 4;
    const EV *__restrict__ v = (const EV *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= p.block_rows * ntiles_n) return; // whole waves only: MFMA needs all 64 lanes
    const long i = wave / ntiles_n;
    const long col0 = (wave % ntiles_n) * 16;
    const int ar = lane & 15, kq = lane >> 4;
    const bool arow_ok = ar < BI;
    const int arc = arow_ok ? ar : 0;
    const long bcol = col0 + (lane & 15);
    const bool bcol_ok = bcol < p.ncols;
    const long bcc = bcol_ok ? bcol : 0;
    acc_t accR = acc_t{0, 0, 0, 0}, accI = acc_t{0, 0, 0, 0};
    const int jb = p.ii[i], je = p.ii[i + 1];
    E an[KS], bn[KS];
    auto fetch = [&](int j) {
        const int dj = p.jj[j];
        const bool ok = dj >= 0;
        const long d0 = ok ? dj : 0;
        const EV *vb = v + (long)j * BI * BD;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int e = ks * 4 + kq;
            const E a = p.block_im_fast ? vb[arc + e * BI] : vb[arc * BD + e];
            const E b = XROW ? x[(d0 + e) * p.ldx + bcc] : x[(d0 + e) + bcc * p.ldx];
            an[ks] = (arow_ok && ok) ? a : E{};
            bn[ks] = bcol_ok ? b : E{};
        }
    };
    if (jb < je) fetch(jb);
    for (int j = jb; j < je; ++j) {
        E af[KS], bf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            af[ks] = an[ks];
            bf[ks] = bn[ks];
        }
        if (j + 1 < je) fetch(j + 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if constexpr (CPLX) {
                accR = BsrMfma<R>::mma(af[ks].x, bf[ks].x, accR);
                accI = BsrMfma<R>::mma(af[ks].x, bf[ks].y, accI);
                accR = BsrMfma<R>::mma(-af[ks].y, bf[ks].y, accR);
                accI = BsrMfma<R>::mma(af[ks].y, bf[ks].x, accI);
            } else {
                accR = BsrMfma<R>::mma(af[ks], bf[ks], accR);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = BsrMfma<R>::row(lane, q);
        if (row >= BI || !bcol_ok) continue;
        const long img = i * BI + row;
        E *yp = YROW ? y + img * p.ldy + bcol : y + img + bcol * p.ldy;
        E out;
        if constexpr (CPLX)
            out = Ops<E>::scale(E{accR[q], accI[q]}, p.alpha_re, p.alpha_im);
        else
            out = Ops<E>::scale(accR[q], p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<E>::add(*yp, out) : out;
    }
}

// ELL form with a compile-time number of nonzero blocks per row (the 9-point stencils): the
// row's block columns are read first (scalar loads), then the fragments of NB blocks at a time
// are loaded one group ahead of the MFMAs, so no load waits on another load and NB blocks' bytes
// are in flight per wave.
template <typename RV, typename R, bool CPLX, int BI, int BD, bool YROW, bool XROW, int NNZ, int NB>
__global__ void __launch_bounds__(256) bsr_mfma_ell_kernel(const BsrArgs p, long ntiles_n) {
    typedef typename BsrMfmaElem<R, CPLX>::type E; // the vectors; the values as stored, widening at the load:
    typedef typename BsrStored<typename BsrMfmaElem<RV, CPLX>::type, E>::type EV;
    typedef typename BsrMfma<R>::acc_t acc_t;
    static_assert(BI <= 16 && BD % 4 == 0 && NNZ % NB == 0, "block shape");
    constexpr int KS = BD / 4, NG = NNZ / NB;
    const EV *__restrict__ v = (const EV *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= p.block_rows * ntiles_n) return; // whole waves only: MFMA needs all 64 lanes
    const long i = wave / ntiles_n;
    const long col0 = (wave % ntiles_n) * 16;
    const int ar = lane & 15, kq = lane >> 4;
    const bool arow_ok = ar < BI;
    const int arc = arow_ok ? ar : 0;
    const long bcol = col0 + (lane & 15);
    const bool bcol_ok = bcol < p.ncols;
    const long bcc = bcol_ok ? bcol : 0;
    const long jb = i * NNZ;
    int dj[NNZ];
#pragma unroll
    for (int k = 0; k < NNZ; ++k) dj[k] = p.jj[jb + k];
    E af[2][NB][KS], bf[2][NB][KS];
    auto fetch = [&](int g, E (*a_)[KS], E (*b_)[KS]) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int k = g * NB + u;
            const bool ok = dj[k] >= 0;
            const long d0 = ok ? dj[k] : 0;
            const EV *vb = v + (jb + k) * (BI * BD);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int e = ks * 4 + kq;
                const E a = p.block_im_fast ? vb[arc + e * BI] : vb[arc * BD + e];
                const E b = XROW ? x[(d0 + e) * p.ldx + bcc] : x[(d0 + e) + bcc * p.ldx];
                a_[u][ks] = (arow_ok && ok) ? a : E{};
                b_[u][ks] = bcol_ok ? b : E{};
            }
        }
    };
    acc_t accR = acc_t{0, 0, 0, 0}, accI = acc_t{0, 0, 0, 0};
    fetch(0, af[0], bf[0]);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) fetch(g + 1, af[(g + 1) & 1], bf[(g + 1) & 1]);
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const E a = af[g & 1][u][ks], b = bf[g & 1][u][ks];
                if constexpr (CPLX) {
                    accR = BsrMfma<R>::mma(a.x, b.x, accR);
                    accI = BsrMfma<R>::mma(a.x, b.y, accI);
                    accR = BsrMfma<R>::mma(-a.y, b.y, accR);
                    accI = BsrMfma<R>::mma(a.y, b.x, accI);
                } else {
                    accR = BsrMfma<R>::mma(a, b, accR);
                }
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = BsrMfma<R>::row(lane, q);
        if (row >= BI || !bcol_ok) continue;
        const long img = i * BI + row;
        E *yp = YROW ? y + img * p.ldy + bcol : y + img + bcol * p.ldy;
        E out;
        if constexpr (CPLX)
            out = Ops<E>::scale(E{accR[q], accI[q]}, p.alpha_re, p.alpha_im);
        else
            out = Ops<E>::scale(accR[q], p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<E>::add(*yp, out) : out;
    }
}

template <typename RV, typename R, bool CPLX, int BI, int BD, int NNZ, int NB>
void launch_bsr_mfma_ell(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s) {
    const long ntn = (a.ncols + 15) / 16;
    const long waves = a.block_rows * ntn;
    const long blocks = (waves + 3) / 4;
    if (blocks >= (1L << 31)) throw Error("bsr: grid too large");
    g_bsr_tune.last = 10;
    KernelTimer timer("bsr", s);
    if (yrow && xrow)
        hipLaunchKernelGGL((bsr_mfma_ell_kernel<RV, R, CPLX, BI, BD, true, true, NNZ, NB>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else if (yrow && !xrow)
        hipLaunchKernelGGL((bsr_mfma_ell_kernel<RV, R, CPLX, BI, BD, true, false, NNZ, NB>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else if (!yrow && xrow)
        hipLaunchKernelGGL((bsr_mfma_ell_kernel<RV, R, CPLX, BI, BD, false, true, NNZ, NB>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else
        hipLaunchKernelGGL((bsr_mfma_ell_kernel<RV, R, CPLX, BI, BD, false, false, NNZ, NB>), dim3(blocks), dim3(256), 0, s, a, ntn);
    SBX_HIP_CHECK(hipGetLastError());
}

template <typename RV, typename R, bool CPLX, int BI, int BD>
void launch_bsr_mfma_pf(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s) {
    const long ntn = (a.ncols + 15) / 16;
    const long waves = a.block_rows * ntn;
    const long blocks = (waves + 3) / 4;
    if (blocks >= (1L << 31)) throw Error("bsr: grid too large");
    g_bsr_tune.last = 11;
    KernelTimer timer("bsr", s);
    if (yrow && xrow)
        hipLaunchKernelGGL((bsr_mfma_pf_kernel<RV, R, CPLX, BI, BD, true, true>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else if (yrow && !xrow)
        hipLaunchKernelGGL((bsr_mfma_pf_kernel<RV, R, CPLX, BI, BD, true, false>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else if (!yrow && xrow)
        hipLaunchKernelGGL((bsr_mfma_pf_kernel<RV, R, CPLX, BI, BD, false, true>), dim3(blocks), dim3(256), 0, s, a, ntn);
    else
        hipLaunchKernelGGL((bsr_mfma_pf_kernel<RV, R, CPLX, BI, BD, false, false>), dim3(blocks), dim3(256), 0, s, a, ntn);
    SBX_HIP_CHECK(hipGetLastError());
}

// Contiguous-block form (row-major x with ldx == ncols <= 16, ELL with NNZ blocks per row): the
// nonzero block A_ij and the x block of its domain rows are each one contiguous run of
// BI*BD (BD*ncols) elements, so a wave moves them by LDS-DMA (buffer_load_dwordx4 ... lds, every
// lane a distinct 16 bytes, 1 KB per instruction, no VGPR round trip) into its LDS slot, PD
// blocks ahead in a ring of PD + 1 slots, instead of 12-row fragment gathers, and reads the MFMA
// fragments from the slot.  (The round-2 register-staged form measured the same on
// complex<double> and 6 % slower on the chain's complex<float> operator, profiles/r02_bsr_blk_sweep.txt.)
// PK > 0 (packed slots): the value block and the x block are one run of the slot (x right after
// the values, no 1-KB rounding of each), moved by PK global_load_lds_dwordx4 instructions whose
// lanes address either array (a buffer load takes one array per instruction) -- 2304 instead of
// 4096 bytes per complex<float> slot at 12 rhs, 4608 instead of 6144 for complex<double>, so more
// waves (and more bytes in flight) fit a CU's LDS
// Mixed products (RV narrower than R: float -> double, f16 -> float): the slot holds the value
// block as it lies in memory, in the operator's type EV (a complex32 block is 576 bytes, a float16
// one 288: less than one DMA instruction), and the x block in E; the fragment reads take EV from
// LDS and widen it (exact) in registers.  The value part's bytes, instruction count and the offset
// of the x part follow from sizeof(EV), the x part's from sizeof(E): unpacked, each part rounded up
// to 1 KB (both parts are 16-byte multiples for every pair); packed, PK = the slot's bytes / 1024
// rounded up, 1..5 by the pair and the column count (complex32 at 12 rhs: 576 + 1152 bytes, PK 2).
// Mixed products take the 4-multiplication complex form.
template <typename RV, typename R, bool CPLX, int BI, int BD, bool YROW, int NNZ, int PD, bool M3, int PK = 0>
__global__ void __launch_bounds__(256) bsr_mfma_dma_kernel(const BsrArgs p, unsigned v_bytes, unsigned x_bytes) {
    typedef typename BsrMfmaElem<R, CPLX>::type E; // the vectors; the values as stored, widening at the load:
    typedef typename BsrStored<typename BsrMfmaElem<RV, CPLX>::type, E>::type EV;
    typedef typename BsrMfma<R>::acc_t acc_t;
    static_assert(BI <= 16 && BD % 4 == 0, "block shape");
    constexpr bool SAME = std::is_same<RV, R>::value;
    static_assert(SAME || !M3, "mixed products: 4 multiplications");
    constexpr int KS = BD / 4, ES = (int)sizeof(E), EVS = (int)sizeof(EV);
    constexpr int ABLK = BI * BD, XBLK = BD * 16;        // elements (x: up to 16 cols)
    static_assert((ABLK * EVS) % 16 == 0, "a value block is whole 16-byte pieces");
    constexpr int NA = (ABLK * EVS + 1023) / 1024, NX = (XBLK * ES + 1023) / 1024; // DMA instructions
    constexpr int NI = PK > 0 ? PK : NA + NX;            // DMA instructions per block
    extern __shared__ __attribute__((aligned(16))) char smem[];
    E *__restrict__ y = (E *)p.y;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long i = (long)blockIdx.x * 4 + w;
    if (i >= p.block_rows) return;
    const int nc = (int)p.ncols, xblk = BD * nc;
    // bytes per ring slot (packed: values then x, 16-byte aligned)
    const unsigned SLOT = PK == 0 ? (unsigned)(NA + NX) * 1024u
                          : SAME  ? (unsigned)(ABLK + xblk) * ES
                                  : (unsigned)(ABLK * EVS + xblk * ES);
    const long jb = i * NNZ;
    int dj[NNZ];
#pragma unroll
    for (int k = 0; k < NNZ; ++k) dj[k] = p.jj[jb + k];
    // the row's NNZ value blocks (one contiguous run) as the buffer: 32-bit offsets at any size
    (void)v_bytes;
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
        (void *)((const EV *)p.v + jb * ABLK), (short)0, NNZ * ABLK * EVS, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void *)p.x, (short)0, (int)x_bytes, 0x00020000);
    const unsigned slot0 = lds_u32(smem) + (unsigned)w * (SLOT * (PD + 1));
    auto issue = [&](int k) {
        const unsigned base = slot0 + (unsigned)(k % (PD + 1)) * SLOT;
        if constexpr (PK > 0) {
            const char *vrow = (const char *)((const EV *)p.v + (jb + k) * ABLK);
            // a skipped block (column -1) reads x's first block row (not used): always BD * nc
            // valid elements, where the block's own values may end before the slot's x part
            const char *xrow = (const char *)((const E *)p.x + (long)(dj[k] < 0 ? 0 : dj[k]) * nc);
#pragma unroll
            for (int q = 0; q < PK; ++q) {
                const unsigned g = (unsigned)(lane + 64 * q) * 16u;
                if (g < SLOT) {
                    const char *src = g < (unsigned)(ABLK * EVS) ? vrow + g : xrow + (g - ABLK * EVS);
                    // nt on the instructions that carry values only (x rows are reused)
                    dma16_lane(src, base + (unsigned)q * 1024u, (p.nt & 1) && (q + 1) * 1024 <= ABLK * EVS);
                }
            }
        } else {
            const unsigned av = (unsigned)(k * ABLK * EVS), xv = (unsigned)((long)(dj[k] < 0 ? 0 : dj[k]) * nc) * ES;
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                const unsigned g = (unsigned)(lane + 64 * q) * 16u;
                dma16(rv, g < (unsigned)(ABLK * EVS) ? av + g : 0x80000000u, base + (unsigned)q * 1024u, p.nt & 1);
            }
#pragma unroll
            for (int q = 0; q < NX; ++q) {
                const unsigned g = (unsigned)(lane + 64 * q) * 16u;
                dma16(rx, g < (unsigned)(xblk * ES) ? xv + g : 0x80000000u, base + (unsigned)(NA + q) * 1024u);
            }
        }
    };
    const int ar = lane & 15, kq = lane >> 4;
    const bool arow_ok = ar < BI, bcol_ok = ar < nc;
    acc_t accR = acc_t{0, 0, 0, 0}, accI = acc_t{0, 0, 0, 0}, acc3 = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PD && k < NNZ; ++k) issue(k);
#pragma unroll
    for (int k = 0; k < NNZ; ++k) {
        // the slot of block k + PD was last read in iteration k - 1: its reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (k + PD < NNZ) issue(k + PD);
        // block k landed: the NI instructions of each later block issued so far may stay in flight
        wait_vmcnt(NI * (NNZ - 1 - k < PD ? NNZ - 1 - k : PD));
        if (dj[k] < 0) continue;
        const EV *sa = (const EV *)(smem + (slot0 - lds_u32(smem)) + (k % (PD + 1)) * SLOT);
        const E *sx = (const E *)(sa + (PK > 0 ? ABLK : NA * 1024 / EVS));
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int e = ks * 4 + kq;
            E a = arow_ok ? (p.block_im_fast ? sa[ar + e * BI] : sa[ar * BD + e]) : E{};
            E b = bcol_ok ? sx[e * nc + ar] : E{};
            if constexpr (CPLX && M3) {
                accR = BsrMfma<R>::mma(a.x, b.x, accR);
                accI = BsrMfma<R>::mma(a.y, b.y, accI);
                acc3 = BsrMfma<R>::mma(a.x + a.y, b.x + b.y, acc3);
            } else if constexpr (CPLX) {
                accR = BsrMfma<R>::mma(a.x, b.x, accR);
                accI = BsrMfma<R>::mma(a.x, b.y, accI);
                accR = BsrMfma<R>::mma(-a.y, b.y, accR);
                accI = BsrMfma<R>::mma(a.y, b.x, accI);
            } else {
                accR = BsrMfma<R>::mma(a, b, accR);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = BsrMfma<R>::row(lane, q);
        if (row >= BI || !bcol_ok) continue;
        const long img = i * BI + row;
        E *yp = YROW ? y + img * p.ldy + ar : y + img + ar * p.ldy;
        E out;
        if constexpr (CPLX && M3)
            out = Ops<E>::scale(E{accR[q] - accI[q], acc3[q] - accR[q] - accI[q]}, p.alpha_re,
                                p.alpha_im);
        else if constexpr (CPLX)
            out = Ops<E>::scale(E{accR[q], accI[q]}, p.alpha_re, p.alpha_im);
        else
            out = Ops<E>::scale(accR[q], p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<E>::add(*yp, out) : out;
    }
}

/// false: not this shape (the register-staged kernel runs)
template <typename R, bool CPLX, int BI, int BD, int NNZ, int PD>
bool launch_bsr_mfma_dma(const BsrArgs &a, bool yrow, hipStream_t s) {
    typedef typename BsrMfmaElem<R, CPLX>::type E;
    constexpr int ES = (int)sizeof(E);
    constexpr int NA = (BI * BD * ES + 1023) / 1024, NX = (BD * 16 * ES + 1023) / 1024;
    const long v_bytes = a.block_rows * NNZ * (long)BI * BD * ES, x_bytes = a.x_rows * a.ldx * (long)ES;
    if (a.x_rows <= 0 || x_bytes >= (1L << 31)) return false;
    const long blocks = (a.block_rows + 3) / 4;
    if (blocks >= (1L << 31)) return false;
    // packed slots (values then x in one run): the DMA instruction count of a block
    const bool m3 = CPLX && g_gemm_tune.m3 > 0;
    const long slot_packed = (long)(BI * BD + BD * a.ncols) * ES;
    // for 8-byte elements only (warm round robin, profiles/r02c_blk_pack.txt: the chain's
    // complex<float> operator 719 -> 693 us; complex<double> 327 -> 336 us)
    const bool want = ES == 8;
    const int pk = want && !m3 ? (int)((slot_packed + 1023) / 1024) : 0;
    // (16-byte aligned pieces: the x blocks of an nc-column row and both arrays)
    const bool packed = pk == (CPLX && ES == 16 ? 5 : 3) && a.ncols >= 1 && a.ncols <= 16 &&
                        (BD * a.ncols * ES) % 16 == 0 && ((size_t)a.x & 15) == 0 &&
                        ((size_t)a.v & 15) == 0;
    const size_t lds = packed ? (size_t)4 * slot_packed * (PD + 1) : (size_t)4 * (NA + NX) * 1024 * (PD + 1);
    // 4 waves x (PD + 1) ring slots; a packed slot's last instruction is masked to the slot
    // (lanes past it are inactive), an unpacked slot is NA + NX whole 64-lane instructions
    if (packed && !m3) {
        // the kernel's issue loop: PKN instructions per slot, lane l of instruction q writes the
        // 16 bytes at q * 1024 + 16 l of the slot when that offset is below the slot size; so a
        // slot's DMA writes min(PKN * 1024, slot rounded up to 16 bytes) bytes and must cover the
        // slot's data, and the ring of 4 waves x (PD + 1) slots, slot_packed bytes apart, must fit
        constexpr long PKN = CPLX && ES == 16 ? 5 : 3;
        const long written = std::min(PKN * 1024, (slot_packed + 15) / 16 * 16);
        if (PKN * 1024 < slot_packed || written > slot_packed)
            throw Error("bsr: internal packed-slot sizing error in bsr_mfma_dma_kernel");
        check_dma_lds("bsr_mfma_dma_kernel", lds, 0, 0, 4L * (PD + 1) * written);
    }
    else
        check_dma_lds("bsr_mfma_dma_kernel", lds, 4L * (PD + 1) * (NA + NX), 64);
    g_bsr_tune.last = packed && !m3 ? 8 : 7;
    KernelTimer timer("bsr", s);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, s, a, (unsigned)v_bytes, (unsigned)x_bytes);
    };
    if (packed && !m3) {
        constexpr int PKN = CPLX && ES == 16 ? 5 : 3;
        if (yrow) go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, true, NNZ, PD, false, PKN>);
        else go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, false, NNZ, PD, false, PKN>);
    } else if (yrow && m3) go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, true, NNZ, PD, true>);
    else if (yrow) go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, true, NNZ, PD, false>);
    else if (m3) go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, false, NNZ, PD, true>);
    else go(bsr_mfma_dma_kernel<R, R, CPLX, BI, BD, false, NNZ, PD, false>);
    SBX_HIP_CHECK(hipGetLastError());
    return true;
}

/// The same for a mixed product (values RV, vectors R).  Only with 16-byte aligned values and x (a
/// DMA lane moves 16 bytes, and a float16 operator may start at any even address) and x blocks that
/// are whole 16-byte pieces; false: not this shape.
///  * form 7, unpacked slots: NA instructions of values (in RV) and NX of x (in R), each a whole
///    64-lane pass of 16 bytes -- lanes past a part's bytes write zeros;
///  * form 8, packed slots: values then x as one run of slot bytes, moved by PK = slot bytes / 1024
///    (rounded up) instructions; the last one is masked to the slot.  PK follows from the pair and
///    the column count (PKMIN..PKMAX: 1 and 16 columns).
/// mixed12_pack 1 packs below 12 columns, where it was measured faster than unpacked slots by more
/// than the spread (16^4 and 16^3 x 64, 1 and 4 columns: 2 % complex32, 8-10 % complex<float> values;
/// at 12 and 16 columns a tie or up to 5 % slower, profiles/bsr_mixed12_measure.txt); 0 never, 2
/// always.
template <typename RV, typename R, bool CPLX, int BI, int BD, int NNZ, int PD>
bool launch_bsr_mfma_dma_mixed(const BsrArgs &a, bool yrow, hipStream_t s) {
    typedef typename BsrMfmaElem<RV, CPLX>::type EV;
    typedef typename BsrMfmaElem<R, CPLX>::type E;
    constexpr int ES = (int)sizeof(E), EVS = (int)sizeof(EV);
    constexpr int NA = (BI * BD * EVS + 1023) / 1024, NX = (BD * 16 * ES + 1023) / 1024;
    constexpr int PKMIN = (BI * BD * EVS + BD * ES + 1023) / 1024, PKMAX = (BI * BD * EVS + BD * 16 * ES + 1023) / 1024;
    static_assert((BI * BD * EVS) % 16 == 0, "a value block is whole 16-byte pieces");
    static_assert(PKMAX <= 5, "wait_vmcnt's counts");
    const long v_bytes = a.block_rows * NNZ * (long)BI * BD * EVS, x_bytes = a.x_rows * a.ldx * (long)ES;
    if (a.x_rows <= 0 || x_bytes >= (1L << 31)) return false;
    const long blocks = (a.block_rows + 3) / 4;
    if (blocks >= (1L << 31)) return false;
    if (a.ncols < 1 || a.ncols > 16 || (BD * a.ncols * ES) % 16 != 0 || ((size_t)a.x & 15) != 0 ||
        ((size_t)a.v & 15) != 0)
        return false;
    KernelTimer timer("bsr", s);
    size_t lds = 0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, s, a, (unsigned)v_bytes, (unsigned)x_bytes);
    };
    if (g_bsr_tune.mixed12_pack >= 2 || (g_bsr_tune.mixed12_pack == 1 && a.ncols < 12)) {
        // the kernel's issue loop: lane l of instruction q writes the 16 bytes at q * 1024 + 16 l of
        // the slot when that offset is below the slot size (a 16-byte multiple): the pk instructions
        // write exactly the slot, every one with a lane in range, in a ring of 4 waves x (PD + 1) slots
        const long slot = (long)BI * BD * EVS + (long)BD * a.ncols * ES;
        const int pk = (int)((slot + 1023) / 1024);
        if (slot % 16 != 0 || pk < PKMIN || pk > PKMAX || (pk - 1) * 1024L >= slot)
            throw Error("bsr: internal packed-slot sizing error in bsr_mfma_dma_kernel (mixed)");
        lds = (size_t)4 * slot * (PD + 1);
        check_dma_lds("bsr_mfma_dma_kernel (mixed, packed)", lds, 0, 0, 4L * (PD + 1) * std::min(pk * 1024L, slot));
        g_bsr_tune.last = 8;
        auto at = [&](auto pkc) {
            constexpr int P = decltype(pkc)::value;
            if constexpr (P >= PKMIN && P <= PKMAX) {
                if (pk == P) {
                    if (yrow) go(bsr_mfma_dma_kernel<RV, R, CPLX, BI, BD, true, NNZ, PD, false, P>);
                    else go(bsr_mfma_dma_kernel<RV, R, CPLX, BI, BD, false, NNZ, PD, false, P>);
                }
            }
        };
        at(std::integral_constant<int, 1>{});
        at(std::integral_constant<int, 2>{});
        at(std::integral_constant<int, 3>{});
        at(std::integral_constant<int, 4>{});
        at(std::integral_constant<int, 5>{});
    } else {
        // 4 waves x (PD + 1) ring slots of NA + NX whole instructions
        lds = (size_t)4 * (NA + NX) * 1024 * (PD + 1);
        check_dma_lds("bsr_mfma_dma_kernel (mixed)", lds, 4L * (PD + 1) * (NA + NX), 64);
        g_bsr_tune.last = 7;
        if (yrow) go(bsr_mfma_dma_kernel<RV, R, CPLX, BI, BD, true, NNZ, PD, false>);
        else go(bsr_mfma_dma_kernel<RV, R, CPLX, BI, BD, false, NNZ, PD, false>);
    }
    SBX_HIP_CHECK(hipGetLastError());
    return true;
}

/// launch_bsr_mfma_dma for either kind of product
template <typename RV, typename R, bool CPLX, int BI, int BD, int NNZ, int PD>
bool launch_bsr_mfma_dma_any(const BsrArgs &a, bool yrow, hipStream_t s) {
    if constexpr (std::is_same<RV, R>::value) return launch_bsr_mfma_dma<R, CPLX, BI, BD, NNZ, PD>(a, yrow, s);
    else return launch_bsr_mfma_dma_mixed<RV, R, CPLX, BI, BD, NNZ, PD>(a, yrow, s);
}

template <typename RV, typename R, bool CPLX, int BI, int BD>
void launch_bsr_mfma(const BsrArgs &a, int nnz, bool yrow, bool xrow, hipStream_t s) {
    // contiguous x blocks (row-major x, ldx == ncols <= 16), 9 blocks per row: the blocks staged
    // by LDS-DMA one ahead (16^4 complex<double> n = 12: 426 us for the round-1 fragment kernel,
    // 348-355 us staged; the chain's complex<float> operator 985 -> 693 us with packed slots;
    // two or three blocks of lookahead were slower, profiles/r02_bsr_blk_sweep.txt; round 6:
    // the value blocks straight into the MFMA fragments with x by LDS-DMA, 757 against 689 us on
    // the chain's operator, and a streaming form with 1-4 workgroups per CU whose waves stream
    // every W-th row through an 8-slot ring, 787-1221 against 695 us -- both removed again,
    // profiles/r06_bsr12_vreg_chain.txt, r06_bsr12_stream_chain.txt, commit ad3532b)
    if (g_bsr_tune.variant == 0 && nnz == 9 && xrow && a.ldx == a.ncols && a.ncols <= 16 &&
        (g_bsr_tune.blk_pd == 2   ? launch_bsr_mfma_dma_any<RV, R, CPLX, BI, BD, 9, 2>(a, yrow, s)
         : g_bsr_tune.blk_pd == 3 ? launch_bsr_mfma_dma_any<RV, R, CPLX, BI, BD, 9, 3>(a, yrow, s)
                                  : launch_bsr_mfma_dma_any<RV, R, CPLX, BI, BD, 9, 1>(a, yrow, s)))
        return;
    // the 9-point stencils otherwise: columns preloaded, fragments one block ahead (a 3- or
    // 9-block lookahead, the XCD-grouped row order and non-temporal value loads were all
    // measured slower, non-temporal stores of y no faster); any other pattern: generic rows
    if (g_bsr_tune.variant != 1 && nnz == 9) return launch_bsr_mfma_ell<RV, R, CPLX, BI, BD, 9, 1>(a, yrow, xrow, s);
    launch_bsr_mfma_pf<RV, R, CPLX, BI, BD>(a, yrow, xrow, s);
}

template <typename E, int BI, int BD, int G>
void launch_ell_g(const BsrArgs &a, int nnz, bool yrow, bool xrow, hipStream_t s, long lds_bytes) {
    const long blk_bytes = (long)nnz * (BI * BD * (long)sizeof(E) + 4);
    const long ngroups = (a.ncols + G - 1) / G;
    int rb = (int)std::max(1L, lds_bytes / std::max(1L, blk_bytes));
    // about one (row, column group) per thread
    if (ngroups <= 256) rb = (int)std::min<long>(rb, std::max(1L, 256 / ngroups));
    const long blocks = (a.block_rows + rb - 1) / rb;
    if (blocks >= (1L << 31)) throw Error("bsr: grid too large");
    const size_t lds = (size_t)rb * blk_bytes;
    KernelTimer timer("bsr", s);
    if (yrow && xrow)
        hipLaunchKernelGGL((bsr_ell_kernel<E, BI, BD, G, true, true>), dim3(blocks), dim3(256), lds, s, a, nnz, rb);
    else if (yrow && !xrow)
        hipLaunchKernelGGL((bsr_ell_kernel<E, BI, BD, G, true, false>), dim3(blocks), dim3(256), lds, s, a, nnz, rb);
    else if (!yrow && xrow)
        hipLaunchKernelGGL((bsr_ell_kernel<E, BI, BD, G, false, true>), dim3(blocks), dim3(256), lds, s, a, nnz, rb);
    else
        hipLaunchKernelGGL((bsr_ell_kernel<E, BI, BD, G, false, false>), dim3(blocks), dim3(256), lds, s, a, nnz, rb);
    SBX_HIP_CHECK(hipGetLastError());
}


// 9-point ELL form of bsr_ell_kernel: each thread reads its block row's 9 block columns straight
// from global memory into registers and issues the x rows of its first PD blocks before the
// workgroup streams the values into LDS, so the x gathers, the column reads and the value stream
// are in flight together (bsr_ell_kernel: value stream, then the columns, then one x block at a
// time); blocks j+PD are fetched while block j is applied.
template <typename E, int BI, int BD, int G, int PD, bool YROW, bool XROW, int NT = 256,
          bool DMAV = false, bool SC = false>
__global__ void __launch_bounds__(NT) bsr_ell9_kernel(const BsrArgs p, int rb) {
    // SC: a thread's G columns are g, g + ngroups, ... (the lanes of one row read consecutive
    // columns in each load) instead of g*G .. g*G + G-1
    // DMAV: the values staged by LDS-DMA (16-byte elements; launcher: 32-bit offsets)
    static_assert(!DMAV || sizeof(E) == 16, "LDS-DMA staging takes 16-byte elements");
    constexpr int NNZ = 9, BLK = BI * BD, NB = PD + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    E *vals = (E *)smem;
    const E *__restrict__ v = (const E *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    // the XCD's range of chunks visited as p.ilv interleaved parts (bsr_ell9_split_kernel)
    const int chunk = xcd_chunk(blockIdx.x, gridDim.x, p.ilv);
    const long row0 = (long)chunk * rb;
    const int nrows = (int)min((long)rb, p.block_rows - row0);
    const long ngroups = (p.ncols + G - 1) / G;
    const long npairs = (long)nrows * ngroups; // <= 256 (launcher)
    const long q = threadIdx.x;
    const bool active = q < npairs;
    int r;
    long g;
    if (YROW) {
        r = (int)(q / ngroups);
        g = q % ngroups;
    } else {
        r = (int)(q % nrows);
        g = q / nrows;
    }
    if (!active) {
        r = 0;
        g = 0;
    }
    long colv[G];
#pragma unroll
    for (int k = 0; k < G; ++k) colv[k] = min(SC ? g + k * ngroups : g * G + k, p.ncols - 1);
    int dj[NNZ];
#pragma unroll
    for (int j = 0; j < NNZ; ++j) dj[j] = p.jj[(row0 + r) * NNZ + j];
    E xb[NB][BD][G];
    auto fetch = [&](int d0, E (*xv)[G]) {
        const long d = d0 < 0 ? 0 : d0;
#pragma unroll
        for (int e = 0; e < BD; ++e)
#pragma unroll
            for (int k = 0; k < G; ++k)
                xv[e][k] = XROW ? x[(d + e) * p.ldx + colv[k]] : x[(d + e) + colv[k] * p.ldx];
    };
#pragma unroll
    for (int j = 0; j < PD; ++j) fetch(dj[j], xb[j]);
    const long vbase = row0 * NNZ * BLK;
    const int nv = nrows * NNZ * BLK;
    if constexpr (DMAV) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)p.v, (short)0, (int)(p.block_rows * NNZ * BLK * 16), 0x00020000);
        const unsigned base = lds_u32(vals) + (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 1024u;
        for (int u = 0; u * NT < nv; ++u) {
            const int e = u * NT + (int)threadIdx.x;
            const unsigned off = e < nv ? (unsigned)((vbase + e) * 16) : 0x80000000u;
            dma16(rs, off, base + (unsigned)(u * NT) * 16u, p.nt & 2);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        for (int e0 = threadIdx.x; e0 < nv; e0 += NT * 8) {
            E t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = v[vbase + min(e0 + NT * u, nv - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (e0 + NT * u < nv) vals[e0 + NT * u] = t[u];
        }
    }
    __syncthreads();
    if (!active) return;
    E acc[BI][G];
#pragma unroll
    for (int c = 0; c < BI; ++c)
#pragma unroll
        for (int k = 0; k < G; ++k) acc[c][k] = Ops<E>::zero();
    const E *vr = vals + r * NNZ * BLK;
#pragma unroll
    for (int j = 0; j < NNZ; ++j) {
        if (j + PD < NNZ) fetch(dj[j + PD], xb[(j + PD) % NB]);
        if (dj[j] < 0) continue;
        const E *vb = vr + j * BLK;
#pragma unroll
        for (int e = 0; e < BD; ++e)
#pragma unroll
            for (int c = 0; c < BI; ++c) {
                const E a = p.block_im_fast ? vb[c + e * BI] : vb[c * BD + e];
#pragma unroll
                for (int k = 0; k < G; ++k)
                    acc[c][k] = Ops<E>::fma(a, xb[j % NB][e][k], acc[c][k]);
            }
    }
#pragma unroll
    for (int c = 0; c < BI; ++c) {
        const long img = (row0 + r) * BI + c;
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const long col = SC ? g + k * ngroups : g * G + k;
            if (col >= p.ncols) break;
            E *yp = YROW ? y + img * p.ldy + col : y + img + col * p.ldy;
            const E out = Ops<E>::scale(acc[c][k], p.alpha_re, p.alpha_im);
            *yp = p.add ? Ops<E>::add(*yp, out) : out;
        }
    }
}

// Site tiles with their halo in LDS (3x3 complex<double> blocks, 9 per row, many rhs columns;
// row-major x and y).  The rows are grouped into tiles of up to TT lattice sites (the host's
// schedule, bsr.cpp: 2x2x2x2 on a 4-d lattice for TT = 16, 2x2x2 for TT = 8) and a tile's distinct
// x rows -- its own sites and their halo, umax at most -- are staged once per slice of NS rhs
// columns into LDS by LDS-DMA (each x row 3 colours x NS columns, NS * 16-byte runs), so the nine
// neighbours of every row are read from LDS instead of nine gathers through the vector-memory
// path (5 staged rows per site instead of 9 fetched ones on the 9-point stencil at TT = 16, 6 at
// TT = 8).  The tile's values (TT x 9 blocks) are staged once and reused by every slice.  Thread
// (site s, colour i, column e) of TT x 3 x NS.
//
// LDS banks (ds_read_b128 serves a wave in four 16-lane groups, MI355X_MICROARCH.md LDS): the x
// piece (slot u, colour d, column e) sits at 16-byte unit u * 3 NS + d NS + e, whose 16-byte bank
// group is (u * 3 NS + d NS + e) mod 16.  NS = 8 (TT = 16): that is 8 ((u + d) mod 2) + e, so two
// sites of one lane group whose neighbour slots have the same parity read the same 8 bank groups:
// 2-way conflicts that depend on the schedule (round 5: 12.6 M conflict cycles per launch at 16^4,
// n = 64).  NS = 16 (TT = 8): the bank group is e alone, and the lane map (s, i, e) puts two sites
// in a lane group only with complementary column sets ({0-3, 12-15} against {4-11}), so no read
// of x conflicts whatever the slots; the colours of a site read the same piece (a broadcast).
struct TileArgs {
    const int *rows;          // [chunk][TT] block rows of the tile (-1: none)
    const int *uniq;          // [chunk][umax] first domain row of each distinct block column (-1: none)
    const unsigned char *loc; // [chunk][TT][9] slot of each nonzero block in uniq (255: skip)
    int umax;
};

// the x DMA passes of a slice: umax * 3 * NS pieces over TT * 3 * NS lanes (the launcher bounds umax)
template <int TT, int NS> struct TileForm {
    static constexpr int NT = TT * 3 * NS;
    static constexpr int UMAX = TT == 16 ? 128 : 80;
    static constexpr int MAXP = (UMAX * 3 * NS + NT - 1) / NT;
};

// Thread (site s, colour i, rhs column e) of TT x 3 x NS.  A slice's y stores are issued after
// the next slice's DMA, so the wait for that DMA (vmcnt(1)) leaves them in flight.
template <bool BIMF, int TT, int NS>
__global__ void __launch_bounds__(TT * 3 * NS) bsr_ell9_tile_kernel(const BsrArgs p, const TileArgs t, int nchunks) {
    typedef double2 E;
    constexpr int NNZ = 9, VP = TT * NNZ * 9, NT = TileForm<TT, NS>::NT; // value pieces (16 B)
    constexpr int MAXP = TileForm<TT, NS>::MAXP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    E *vals = (E *)smem;
    E *xs = vals + VP;
    const int tid = threadIdx.x, w = tid >> 6;
    // XCD-contiguous ranges of tiles: neighbouring tiles share halo rows in that XCD's L2
    const int chunk = xcd_chunk(blockIdx.x, gridDim.x);
    if (chunk >= nchunks) return;
    const int umax = t.umax, XP = umax * 3 * NS; // x pieces of a slice
    const int *rows = t.rows + (long)chunk * TT;
    const int *uq = t.uniq + (long)chunk * umax;
    const unsigned char *lc = t.loc + (long)chunk * TT * NNZ;
    const unsigned vbase = lds_u32(vals), xbase = lds_u32(xs);
    // the values of the tile's rows (read once: nt)
    const E *v = (const E *)p.v;
    for (int u = 0; u * NT < VP; ++u) {
        const int L = u * NT + tid;
        if (L < VP) {
            const int s = L / 81, r = rows[s];
            dma16_lane(v + (long)(r < 0 ? 0 : r) * 81 + (L - s * 81),
                       vbase + (unsigned)(u * NT + w * 64) * 16u, (p.nt & 2) != 0);
        }
    }
    // this lane's x pieces (pass u: distinct row pu, colour pd, column pe), the same every slice
    // (element offsets into x: 32 bits, the launcher checks x's size)
    unsigned src[MAXP];
    const E *x = (const E *)p.x;
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
        const int L = u * NT + tid;
        const int pu = L / (3 * NS), rem = L - pu * 3 * NS, pd = rem / NS, pe = rem - pd * NS;
        const int d = (L < XP) ? uq[L < XP ? pu : 0] : -1; // (the index clamped: no load past the list)
        src[u] = (unsigned)(((long)(d < 0 ? 0 : d) + pd) * p.ldx + pe);
    }
    auto stage = [&](int q) {
#pragma unroll
        for (int u = 0; u < MAXP; ++u) {
            const int L = u * NT + tid;
            if (u * NT < XP && L < XP)
                dma16_lane(x + src[u] + q * NS, xbase + (unsigned)(u * NT + w * 64) * 16u, false);
        }
    };
    // this thread's output and its nine slots
    const int e = tid % NS, i = (tid / NS) % 3, s = tid / (3 * NS);
    const int row = rows[s];
    const bool wave_stores = __ballot(row >= 0) != 0;
    int slot[NNZ];
#pragma unroll
    for (int k = 0; k < NNZ; ++k) slot[k] = lc[s * NNZ + k];
    const E *vr = vals + s * NNZ * 9;
    E *y = (E *)p.y;
    const int nslices = (int)(p.ncols / NS);
    stage(0);
    for (int q = 0; q < nslices; ++q) {
        // slice q landed (only the previous slice's y store, issued after it, may be pending; a
        // wave whose rows are all padding stores nothing: it waits for everything)
        if (q == 0 || !wave_stores) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        __syncthreads();
        E acc = Ops<E>::zero();
#pragma unroll
        for (int k = 0; k < NNZ; ++k) {
            if (slot[k] == 255) continue;
            const E *xr = xs + slot[k] * 3 * NS + e;
            const E *vb = vr + k * 9;
#pragma unroll
            for (int d = 0; d < 3; ++d) acc = Ops<E>::fma(BIMF ? vb[i + d * 3] : vb[i * 3 + d], xr[d * NS], acc);
        }
        __syncthreads(); // every read of the buffer is done
        if (q + 1 < nslices) stage(q + 1);
        if (row >= 0) {
            E *yp = y + ((long)row * 3 + i) * p.ldy + q * NS + e;
            const E out = Ops<E>::scale(acc, p.alpha_re, p.alpha_im);
            *yp = p.add ? Ops<E>::add(*yp, out) : out;
        }
    }
}

/// false: no tile schedule, not this shape, or bsr.tile off.  bsr.tile 1: 16-site tiles, slices
/// of 8 columns (schedule 0); 2: 8-site tiles, slices of 16 columns (schedule 1)
bool launch_ell9_tile(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s) {
    const int form = g_bsr_tune.tile;
    if (form != 1 && form != 2) return false;
    const TileSched &ts = a.tiles[form - 1];
    const int NS = form == 1 ? 8 : 16, TT = form == 1 ? 16 : 8;
    const int umax_cap = form == 1 ? TileForm<16, 8>::UMAX : TileForm<8, 16>::UMAX;
    if (!ts.rows || ts.tt != TT || !yrow || !xrow || a.ncols % NS != 0 || ts.umax < 1 ||
        ts.umax > umax_cap || ts.chunks >= (1L << 31) || a.ldx < a.ncols || a.ldy < a.ncols ||
        a.x_rows <= 0 || a.x_rows * a.ldx >= (1L << 32))
        return false;
    const TileArgs t{ts.rows, ts.uniq, ts.loc, ts.umax};
    const long vp = TT * 9L * 9, xp = ts.umax * 3L * NS;
    const size_t lds = (size_t)(vp + xp) * 16;
    // the DMA passes write lanes L < vp (values) and L < xp (x) only
    check_dma_lds("bsr_ell9_tile_kernel", lds, 1, vp + xp);
    g_bsr_tune.last = form == 1 ? 4 : 13;
    KernelTimer timer("bsr", s);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)ts.chunks), dim3(TT * 3 * NS), lds, s, a, t, (int)ts.chunks);
    };
    if (form == 1) {
        if (a.block_im_fast) go(bsr_ell9_tile_kernel<true, 16, 8>);
        else go(bsr_ell9_tile_kernel<false, 16, 8>);
    } else {
        if (a.block_im_fast) go(bsr_ell9_tile_kernel<true, 8, 16>);
        else go(bsr_ell9_tile_kernel<false, 8, 16>);
    }
    SBX_HIP_CHECK(hipGetLastError());
    return true;
}

template <typename E, int BI, int BD, int G, int PD, int NT = 256, bool DMAV = false, bool SC = false>
void launch_ell9(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s, long lds_bytes) {
    const long blk_bytes = 9L * BI * BD * (long)sizeof(E);
    const long ngroups = (a.ncols + G - 1) / G;
    if (ngroups > NT) throw Error("bsr: internal ELL9 sizing error");
    int rb = (int)std::max(1L, lds_bytes / blk_bytes);
    rb = (int)std::min<long>(rb, std::max(1L, NT / ngroups));
    const long blocks = (a.block_rows + rb - 1) / rb;
    if (blocks >= (1L << 31)) throw Error("bsr: grid too large");
    if constexpr (DMAV)
        if (a.block_rows * blk_bytes >= (1L << 31)) return launch_ell9<E, BI, BD, G, PD, NT, false, SC>(a, yrow, xrow, s, lds_bytes);
    // the DMA form fills whole workgroup-wide rows of 16-byte lanes
    const size_t lds = DMAV ? (size_t)((rb * 9L * BI * BD + NT - 1) / NT * NT) * sizeof(E)
                            : (size_t)rb * blk_bytes;
    // the DMA loop: passes u < ceil(nv / NT) of NT lanes, nv <= rb * 81 (the last chunk fewer)
    if constexpr (DMAV) check_dma_lds("bsr_ell9_kernel", lds, (rb * 9L * BI * BD + NT - 1) / NT, NT);
    g_bsr_tune.last = 3;
    KernelTimer timer("bsr", s);
    if (yrow && xrow)
        hipLaunchKernelGGL((bsr_ell9_kernel<E, BI, BD, G, PD, true, true, NT, DMAV, SC>), dim3(blocks), dim3(NT), lds, s, a, rb);
    else if (yrow && !xrow)
        hipLaunchKernelGGL((bsr_ell9_kernel<E, BI, BD, G, PD, true, false, NT, DMAV, SC>), dim3(blocks), dim3(NT), lds, s, a, rb);
    else if (!yrow && xrow)
        hipLaunchKernelGGL((bsr_ell9_kernel<E, BI, BD, G, PD, false, true, NT, DMAV, SC>), dim3(blocks), dim3(NT), lds, s, a, rb);
    else
        hipLaunchKernelGGL((bsr_ell9_kernel<E, BI, BD, G, PD, false, false, NT, DMAV, SC>), dim3(blocks), dim3(NT), lds, s, a, rb);
    SBX_HIP_CHECK(hipGetLastError());
}

// Few rhs columns (n <= NC <= 4), 3x3 blocks, 9 per row: one thread per (block row, nonzero
// block).  The value stream is read by 9 x more threads than in the row-chunk kernel, without
// an LDS staging pass, and every thread has a single x gather (its block's domain rows) in
// flight beside its 9 values; the 9 partial products of a row are summed through LDS in block
// order.  At n = 1 the row-chunk kernel keeps one thread per row busy through 9 dependent
// gathers (18 of 256 threads of a workgroup active).
template <typename E, int NC, bool YROW, bool XROW, bool DMA>
__global__ void __launch_bounds__(256) bsr_ell9_row_kernel(const BsrArgs p, unsigned v_bytes) {
    constexpr int NNZ = 9, BI = 3, BD = 3, BLK = 9, RW = 28; // 28 rows x 9 blocks = 252 threads
    constexpr int NV = RW * NNZ * BLK, NP = RW * NNZ * BI * NC;
    constexpr int NS = (DMA ? (NV + 255) / 256 * 256 : 0) > NP ? (NV + 255) / 256 * 256 : NP;
    // static LDS: every DMA pass (256 lanes, the last one partly zeros) and the partial products
    static_assert((!DMA || NS >= (NV + 255) / 256 * 256) && NS >= NP, "LDS sizing");
    __shared__ __attribute__((aligned(16))) E sh[NS]; // values (DMA), then the partial products
    const E *__restrict__ v = (const E *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const long chunk = xcd_chunk(blockIdx.x, gridDim.x);
    const int tid = threadIdx.x, rl = tid / NNZ, j = tid - rl * NNZ;
    const long row = chunk * RW + rl;
    const int ncols = (int)p.ncols;
    const bool active = rl < RW && row < p.block_rows;
    const long q = row * NNZ + j;
    int dj = -1;
    E xv[BD][NC];
    if (active) {
        dj = p.jj[q];
        const long d = dj < 0 ? 0 : dj;
#pragma unroll
        for (int e = 0; e < BD; ++e)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const long col = c < ncols ? c : 0;
                xv[e][c] = XROW ? x[(d + e) * p.ldx + col] : x[(d + e) + col * p.ldx];
            }
    }
    E a[BLK];
    if constexpr (DMA) {
        // the chunk's values, lane-linear into LDS (a contiguous run of the ELL value array)
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void *)p.v, (short)0, (int)v_bytes, 0x00020000);
        const unsigned base = lds_u32(sh) + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6) * 1024u;
        const unsigned v0 = (unsigned)(chunk * NV) * 16u;
#pragma unroll
        for (int u = 0; u < (NV + 255) / 256; ++u) {
            const unsigned e = (unsigned)(u * 256 + tid);
            const unsigned off = e < (unsigned)NV ? v0 + e * 16u : 0x80000000u;
            dma16(rs, off, base + (unsigned)u * 4096u, p.nt & 8);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (active) {
#pragma unroll
            for (int k = 0; k < BLK; ++k) a[k] = sh[(rl * NNZ + j) * BLK + k];
        }
        __syncthreads(); // the buffer now holds the partial products
    } else if (active) {
#pragma unroll
        for (int k = 0; k < BLK; ++k) a[k] = v[q * BLK + k];
    }
    E *part = sh;
    if (active) {
#pragma unroll
        for (int i = 0; i < BI; ++i)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                E acc = Ops<E>::zero();
#pragma unroll
                for (int e = 0; e < BD; ++e)
                    acc = Ops<E>::fma(p.block_im_fast ? a[i + e * BI] : a[i * BD + e], xv[e][c], acc);
                part[((rl * NNZ + j) * BI + i) * NC + c] = dj < 0 ? Ops<E>::zero() : acc;
            }
    }
    __syncthreads();
    // sums: one thread per (row, i, column)
    for (int o = tid; o < RW * BI * ncols; o += 256) {
        const int r2 = o / (BI * ncols), rem = o - r2 * BI * ncols, i = rem / ncols, c = rem - i * ncols;
        const long rw = chunk * RW + r2;
        if (rw >= p.block_rows) continue;
        E acc = part[((r2 * NNZ) * BI + i) * NC + c];
#pragma unroll
        for (int jj = 1; jj < NNZ; ++jj) acc = Ops<E>::add(acc, part[((r2 * NNZ + jj) * BI + i) * NC + c]);
        const long img = rw * BI + i;
        E *yp = YROW ? y + img * p.ldy + c : y + img + (long)c * p.ldy;
        const E out = Ops<E>::scale(acc, p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<E>::add(*yp, out) : out;
    }
}

template <typename E, int NC>
void launch_ell9_row(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s) {
    const long blocks = (a.block_rows + 27) / 28;
    if (blocks >= (1L << 31)) throw Error("bsr: grid too large");
    // the LDS-DMA form for 16-byte elements whose value array has 32-bit offsets
    const long v_bytes = a.block_rows * 81L * (long)sizeof(E);
    const bool dma = sizeof(E) == 16 && v_bytes < (1L << 31);
    g_bsr_tune.last = 1;
    KernelTimer timer("bsr", s);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a, (unsigned)v_bytes);
    };
    if (dma) {
        if (yrow && xrow) go(bsr_ell9_row_kernel<E, NC, true, true, true>);
        else if (yrow && !xrow) go(bsr_ell9_row_kernel<E, NC, true, false, true>);
        else if (!yrow && xrow) go(bsr_ell9_row_kernel<E, NC, false, true, true>);
        else go(bsr_ell9_row_kernel<E, NC, false, false, true>);
    } else {
        if (yrow && xrow) go(bsr_ell9_row_kernel<E, NC, true, true, false>);
        else if (yrow && !xrow) go(bsr_ell9_row_kernel<E, NC, true, false, false>);
        else if (!yrow && xrow) go(bsr_ell9_row_kernel<E, NC, false, true, false>);
        else go(bsr_ell9_row_kernel<E, NC, false, false, false>);
    }
    SBX_HIP_CHECK(hipGetLastError());
}

// Rows split over their nonzero blocks, 3x3 complex<double> blocks, 9 per row, row-major x, from
// 4 rhs columns on: one thread per (block row, group of JB nonzero blocks, rhs lane g), the lane
// computing columns g, g + nct, ... (CW of them; nct = ceil(ncols / CW) lanes per block group).
//  * Every thread issues the x rows of its JB blocks at once (JB x 3 x CW independent 16-byte
//    loads, no chain of dependent gathers), the nct lanes of a block group read whole runs of a
//    domain row (12 columns: 192 B pieces; the row-chunk kernel's lanes read 96 B pieces, which
//    the vector-memory pipeline serves ~1.4x slower from the Infinity Cache,
//    tools/gather_shape.hip), through 32-bit buffer offsets (one multiply per block instead of
//    six 64-bit address computations).
//  * The workgroup's block values (one contiguous run) are staged by LDS-DMA and read from LDS,
//    broadcast across the lanes of a block group.
//  * The 9 / JB partial products of a row are summed through LDS in block order.
__device__ __forceinline__ unsigned fdiv(unsigned n, unsigned m, int s) {
    return (unsigned)(((unsigned long long)__umulhi(n, m) + n) >> s);
}

static void magic(unsigned d, unsigned &m, int &s) {
    s = 0;
    while ((1ull << s) < d) ++s;
    m = (unsigned)((((1ull << 32) * ((1ull << s) - d)) / d) + 1);
}

struct SplitArgs {
    int nct, tpr, rw; // lanes per block group, threads per row, rows per workgroup
    unsigned v_bytes, x_bytes;
    unsigned tpr_m, nct_m; // magic multipliers and shifts of tpr and nct (fdiv)
    int tpr_s, nct_s;
    int ilv; // an XCD's chunks visited as ilv interleaved parts (x rows reused across parts)
    int ovl; // the partial products overwrite the staged values (one more barrier, half the LDS)
};

template <int CW, int JB, bool YROW>
__global__ void __launch_bounds__(512) bsr_ell9_split_kernel(const BsrArgs p, const SplitArgs s) {
    constexpr int NNZ = 9, NG = NNZ / JB;
    static_assert(NNZ % JB == 0, "JB divides 9");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2 *vals = (double2 *)smem;
    const int nth = blockDim.x, tid = threadIdx.x;
    // the XCD's contiguous range of chunks, its parts interleaved: with ilv = 2 the two halves
    // (on the 16^4 lattice: the XCD's two x slices) are visited together, so a site's +-x
    // neighbour rows are read while the other half still holds them in this XCD's L2
    const long chunk = xcd_chunk(blockIdx.x, gridDim.x, s.ilv);
    const long row0 = chunk * s.rw;
    const int nrows = (int)min((long)s.rw, p.block_rows - row0);
    const int nv = nrows * NNZ * 9, nvp = (s.rw * NNZ * 9 + nth - 1) / nth * nth;
    double2 *part = s.ovl ? vals : vals + nvp;
    const int rl = (int)fdiv(tid, s.tpr_m, s.tpr_s), rem = tid - rl * s.tpr;
    const int jg = (int)fdiv(rem, s.nct_m, s.nct_s), g = rem - jg * s.nct;
    const bool active = rl < nrows;
    const int ncs = s.nct * CW; // padded columns of a partial-product row
    // 1) the x rows of the thread's JB blocks
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void *)p.x, (short)0, (int)s.x_bytes, 0x00020000);
    const unsigned rowb = (unsigned)p.ldx * 16u;
    int dj[JB];
    double2 xv[JB][3][CW];
#pragma unroll
    for (int b = 0; b < JB; ++b) dj[b] = active ? p.jj[(row0 + rl) * NNZ + jg * JB + b] : -1;
    // the lane's columns, clamped to the last one (the surplus lanes' results are not stored)
    unsigned colb[CW];
#pragma unroll
    for (int k = 0; k < CW; ++k) colb[k] = (unsigned)min(g + k * s.nct, (int)p.ncols - 1) * 16u;
#pragma unroll
    for (int b = 0; b < JB; ++b) {
        // skipped blocks (-1) read zero beyond the buffer range; the block's 3 domain rows by the
        // uniform offset e * rowb
        const unsigned vb = dj[b] < 0 ? 0x80000000u : (unsigned)dj[b] * rowb;
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
            for (int k = 0; k < CW; ++k) {
                const auto t = __builtin_amdgcn_raw_buffer_load_b128(rx, vb + colb[k], (unsigned)e * rowb, 0);
                xv[b][e][k] = __builtin_bit_cast(double2, t);
            }
    }
    // 2) the workgroup's block values, lane-linear into LDS
    {
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void *)p.v, (short)0, (int)s.v_bytes, 0x00020000);
        const unsigned base = lds_u32(vals) + (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6) * 1024u;
        const unsigned v0 = (unsigned)(row0 * NNZ * 9) * 16u;
        for (int u = 0; u * nth < nv; ++u) {
            const int e = u * nth + tid;
            const unsigned off = e < nv ? v0 + (unsigned)e * 16u : 0x80000000u;
            dma16(rs, off, base + (unsigned)(u * nth) * 16u, p.nt & 4);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // 3) the partial products of the thread's blocks
    double2 acc[3][CW];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < CW; ++k) acc[c][k] = double2{0, 0};
    if (active) {
#pragma unroll
        for (int b = 0; b < JB; ++b) {
            if (dj[b] < 0) continue;
            const double2 *vb = vals + (rl * NNZ + jg * JB + b) * 9;
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double2 a = p.block_im_fast ? vb[c + e * 3] : vb[c * 3 + e];
#pragma unroll
                    for (int k = 0; k < CW; ++k) acc[c][k] = Ops<double2>::fma(a, xv[b][e][k], acc[c][k]);
                }
        }
    }
    auto store = [&](long img, int col, double2 v) {
        double2 *yp = YROW ? (double2 *)p.y + img * p.ldy + col : (double2 *)p.y + img + (long)col * p.ldy;
        const double2 out = Ops<double2>::scale(v, p.alpha_re, p.alpha_im);
        *yp = p.add ? Ops<double2>::add(*yp, out) : out;
    };
    if constexpr (NG == 1) {
        if (!active) return;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < CW; ++k) {
                const int col = g + k * s.nct;
                if (col < p.ncols) store((row0 + rl) * 3 + c, col, acc[c][k]);
            }
    } else {
        if (s.ovl) __syncthreads(); // every thread is done reading the values
        if (active) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < CW; ++k) part[((rl * NG + jg) * 3 + c) * ncs + g + k * s.nct] = acc[c][k];
        }
        __syncthreads();
        // 4) sums in block order: the lanes of block group c < 3 sum image component c
        if (!active || jg >= 3) return;
#pragma unroll
        for (int k = 0; k < CW; ++k) {
            const int col = g + k * s.nct;
            if (col >= p.ncols) break;
            const double2 *pp = part + ((rl * NG) * 3 + jg) * ncs + col;
            double2 sum = pp[0];
#pragma unroll
            for (int q = 1; q < NG; ++q) sum = Ops<double2>::add(sum, pp[q * 3 * ncs]);
            store((row0 + rl) * 3 + jg, col, sum);
        }
    }
}

/// false: not this shape (the caller falls back to the row-chunk kernel)
template <typename E>
bool launch_ell9_split(const BsrArgs &a, bool yrow, bool xrow, hipStream_t st) {
    if constexpr (!std::is_same<E, double2>::value) {
        return false;
    } else {
        if (!xrow || a.ncols < 1) return false;
        const long x_bytes = a.x_rows * a.ldx * 16L;
        const long v_bytes = a.block_rows * 81L * 16L;
        if (v_bytes >= (1L << 31) || a.block_rows * 36L >= (1L << 31)) return false;
        if (a.x_rows <= 0 || x_bytes >= (1L << 31)) return false;
        // defaults from tools/bsr_split_sweep.py (16^4, profiles/r02_bsr_split_sweep.txt)
        int cw = g_bsr_tune.split_cw;
        if (cw <= 0) cw = a.ncols <= 4 ? 1 : 2;
        int jb = g_bsr_tune.split_jb;
        if (jb <= 0) jb = a.ncols <= 24 ? 3 : 9;
        // the forms the defaults use (the sweep's other forms were slower everywhere)
        if ((cw != 1 && cw != 2) || (jb != 3 && jb != 9)) return false;
        const int nct = (int)((a.ncols + cw - 1) / cw), tpr = 9 / jb * nct;
        const int ntmax = 256; // 512-thread workgroups measured slower (profiles/r02c_split_ovl.txt)
        if (tpr > ntmax) return false;
        // rows per workgroup: by the thread budget and at most 40 KB of LDS; the partial products
        // overlay the staged values (one more barrier, four workgroups per CU instead of three)
        const bool ovl = true;
        const long part_row = jb == 9 ? 0L : (long)(9 / jb) * 3 * nct * cw * 16;
        const long row_lds = std::max(81L * 16, part_row);
        const int rw = std::max(1, std::min<int>(ntmax / tpr, (int)(40960 / row_lds)));
        const int nth = (rw * tpr + 63) / 64 * 64;
        const long nvp = (rw * 81L + nth - 1) / nth * nth;
        const long npart = jb == 9 ? 0L : (long)rw * (9 / jb) * 3 * nct * cw;
        const long lds = (ovl ? std::max(nvp, npart) : nvp + npart) * 16L;
        if (lds > 65536) return false;
        // DMA passes u < ceil(nv / nth) of nth lanes (nv <= rw * 81); the partial products
        // overlay them (ovl) or follow them
        check_dma_lds("bsr_ell9_split_kernel", (size_t)lds, (rw * 81L + nth - 1) / nth, nth,
                      ovl ? 0 : npart * 16);
        check_dma_lds("bsr_ell9_split_kernel partials", (size_t)lds, 0, 0,
                      (ovl ? 0 : nvp * 16) + npart * 16);
        SplitArgs sa{nct, tpr, rw, (unsigned)v_bytes, (unsigned)x_bytes, 0, 0, 0, 0,
                     std::max(1, g_bsr_tune.split_ilv), ovl ? 1 : 0};
        magic((unsigned)tpr, sa.tpr_m, sa.tpr_s);
        magic((unsigned)nct, sa.nct_m, sa.nct_s);
        const long nchunks = (a.block_rows + rw - 1) / rw;
        if (nchunks >= (1L << 31)) return false;
        g_bsr_tune.last = 2;
        KernelTimer timer("bsr", st);
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(nchunks), dim3(nth), (size_t)lds, st, a, sa); };
#define SBX_SPLIT(CW_, JB_)                                                                        \
    if (cw == CW_ && jb == JB_) {                                                                  \
        if (yrow) go(bsr_ell9_split_kernel<CW_, JB_, true>);                                       \
        else go(bsr_ell9_split_kernel<CW_, JB_, false>);                                           \
    }
        SBX_SPLIT(1, 3) SBX_SPLIT(1, 9) SBX_SPLIT(2, 3) SBX_SPLIT(2, 9)
#undef SBX_SPLIT
        SBX_HIP_CHECK(hipGetLastError());
        return true;
    }
}

template <typename E, int BI, int BD>
void launch_ell(const BsrArgs &a, int nnz, bool yrow, bool xrow, hipStream_t s) {
    // two rhs columns per thread (measured against 1 and 4, and 48 KB of LDS per workgroup:
    // 16^4 3x3 n = 12: 46 us vs 51 / 61; n = 64: 191 us vs 218 / 234; one column per thread
    // over all 256 threads with the x rows of all 9 blocks in flight: 56-60 us; non-temporal
    // loads of the value stream: 50 us)
    // the 9-point stencils: ell9 with 12 KB of values per workgroup from 8 rhs columns on, else
    // 24 KB (16^4 3x3: n = 1 30.6 -> 26.5 us, n = 4 33.3 -> 28.1, n = 12 47.3 -> 42.9, n = 64
    // 190 -> 181-188; at n = 12 6 / 8 / 16 / 24 KB: 72 / 52 / 48 / 45 us; one or four columns
    // per thread, or the x rows of two blocks ahead: 46-82 us).  The x gathers are the bound:
    // without them the value stream and y run at 5.5 TB/s (22 us at n = 12).
    if constexpr (BI == 3 && BD == 3) {
        if (nnz == 9 && g_bsr_tune.variant != 1 && a.ncols <= g_bsr_tune.row_max_cols) {
            if (a.ncols == 1) return launch_ell9_row<E, 1>(a, yrow, xrow, s);
            if (a.ncols == 2) return launch_ell9_row<E, 2>(a, yrow, xrow, s);
            if (a.ncols <= 4) return launch_ell9_row<E, 4>(a, yrow, xrow, s);
        }
        if (nnz == 9 && g_bsr_tune.variant != 1 && a.ncols > g_bsr_tune.row_max_cols &&
            a.ncols <= g_bsr_tune.split_max_cols && launch_ell9_split<E>(a, yrow, xrow, s))
            return;
    }
    if constexpr (std::is_same<E, double2>::value && BI == 3 && BD == 3) {
        if (nnz == 9 && g_bsr_tune.variant != 1 && g_bsr_tune.tile && a.ncols >= g_bsr_tune.tile_min_cols &&
            launch_ell9_tile(a, yrow, xrow, s))
            return;
    }
    // (the row-chunk kernel takes at most 2 x 256 rhs columns per workgroup row)
    if (nnz == 9 && g_bsr_tune.variant != 1 && a.ncols <= 512) {
        const long lds = a.ncols >= 8 ? 12288 : 24576;
        // 16-byte elements: values by LDS-DMA, a row's lanes on consecutive columns (n = 12:
        // 42 -> 39 us, n = 24: 67 -> 61, n = 64: 182 -> 172; profiles/r02_bsr_sweep.txt; 64- and
        // 128-thread workgroups, two blocks of x lookahead, non-temporal value loads or y stores
        // were slower)
        if constexpr (sizeof(E) == 16) return launch_ell9<E, BI, BD, 2, 1, 256, true, true>(a, yrow, xrow, s, lds);
        else return launch_ell9<E, BI, BD, 2, 1>(a, yrow, xrow, s, lds);
    }
    launch_ell_g<E, BI, BD, 2>(a, nnz, yrow, xrow, s, ELL_LDS_BYTES);
}

// Dense blocks of 16 x 16 and more (the multigrid coarse operators: (2 nv) x (2 nv) blocks, 9
// per row, 1-64 rhs columns) on the matrix cores.  One workgroup per block row and group of NT
// tiles of 16 rhs columns; wave w owns the 16-row strip w % nstrips of the row (at most 8
// strips, bi <= 128).  Per nonzero block:
//  * the workgroup stages the bd x 16 NT piece of x once into LDS (any x layout; rows past bd
//    and columns past ncols as zeros), one block ahead in two buffers, so one barrier per block.
//    The LDS image keeps the VE = 16 / sizeof(E) consecutive k of a column together: a B
//    fragment of VE k-steps is one 16-byte LDS read;
//  * a wave reads its strip of the value block straight into A fragments: lane (row r, k-group
//    kq) takes the VA consecutive k at (4 ss + kq) VA of row r as one 16-byte load (row-major
//    blocks whose rows are 16-byte multiples; the k order inside a block is free, A and B
//    agree on it), four such loads in flight -- a block's first four issued before the next x
//    block is staged (48x48 complex<float> n = 12: 203 -> 188 us) -- and applies them to all NT
//    column tiles: the values are read once per group of NT tiles.  Blocks stored image-fastest (block_im_fast)
//    are read as 16-element column runs, ragged tails element by element, never past the block;
//  * rows of one or two strips split the k-steps of a block over 4 / 2 waves (kparts); the
//    partial tiles are summed through LDS in wave order, so the result has one fixed order.
// No LDS-DMA (no check_dma_lds), no atomics; every offset into v, x and y is 64-bit; the 16-byte
// value load only where all of it lies inside the row (k0 + VA <= bd) of an aligned operator,
// else by elements.
//
// The one kernel serves three forms (bsr.last_kernel), the differences under if constexpr:
//  * 14, the same-type product: values and vectors of type E = (R, CPLX), VA = VE, H = 1;
//  * 16, the mixed product (RV = float, R = double): an operator kept in single precision
//    applied to double-precision vectors on v_mfma_f64_16x16x4_f64.  The value fragments are
//    read in the operator's type EV: lane (row r, k-group kq) reads the VA = 16 / sizeof(EV)
//    consecutive k at (4 ss + kq) VA of row r as one 16-byte load (2 complex<float>, 4 float) and
//    widens them (exact) in registers just before the MFMAs, so a fragment in flight is 4 VGPRs
//    as in the same-type product; no converted copy of the values exists.  x is staged in LDS as
//    doubles and B keeps A's k order: lane (column c, kq) takes the same VA k of column c, 32
//    bytes, as H = VA / VE = 2 16-byte reads.  LDS banks (ds_read_b128 serves a wave in four
//    16-lane groups, each holding every column once with two values of kq; bank (a / 4) mod 64,
//    a 256-byte row of sixteen 16-byte slots): with the 32 bytes adjacent, a read's slot is
//    2 c (+ 1) mod 16 -- columns c and c + 8 of a lane group on one slot, a 2-way conflict on
//    every read.  So the H pieces of a group lie XW slots apart, image [k-group][piece][column]:
//    the slot of a read is c mod 16, every lane group covers the 16 slots once, no conflict.
//    (For either pair that is the same-type image of the double type; H = 1 gives form 14's.)
//    The same form with RV = f16, R = float: an operator kept in half precision applied to
//    single-precision vectors on v_mfma_f32_16x16x4_f32.  A lane's 16-byte value load is VA = 4
//    complex-half or 8 half consecutive k, widened (exact: v_cvt_f32_f16) in registers; x is
//    staged as float2 / float, VE = 2 / 4, so again H = VA / VE = 2 and a k-step is 4 VA = 16
//    (complex) or 32 (real) k -- kpad, kparts and the ragged tails follow from VA alone.  The
//    bank argument above counts 16-byte slots and never the element size: a piece is one slot
//    whether it holds 1 double2, 2 float2 or 4 float, element k of column c lies in slot
//    (k / VE) XW + c = ((k / VA) H + (k % VA) / VE) XW + c, XW is a multiple of 16, and so the
//    slot of lane (c, kq)'s read h is c mod 16 for 8- and 4-byte elements too: every 16-lane
//    group of a ds_read_b128 covers the 16 slots of the bank row once.  (The staging stores are
//    form 14's for float2 / float, one element each.)
//  * 17, ADJ, the in-place adjoint (bsr.adj_inplace): the transposed operator's pattern over A's
//    own value array.  Entry j of a block row reads block ent[j] of A instead of block j of the
//    copy, and the imaginary parts are negated in registers as a fragment is loaded (real types
//    load unchanged; the zeros of the padding are never loaded and stay as they are): the bytes
//    read per block are the copy's, plus the 4 of ent[j].  The block is A's storage read in the
//    flipped order (p.block_im_fast is the opposite of A's), so A's row-major blocks are the
//    image-fastest case here, exactly as on the copy, and the 16-byte loads apply where they
//    would on the copy and A's array is 16-byte aligned.  Entries are in ascending nonzero index
//    of A within a block column, the copy's order; the conjugation is an exact sign flip and
//    every other operation is the same, so the result has the bits of form 14 on the copy.
//    (The template also expresses the mixed in-place adjoint; it is neither instantiated nor
//    dispatched: mixed pairs take the generic form 18.)
template <typename E> struct alignas(16) BlkVec { E e[16 / sizeof(E)]; };

template <typename RV, typename R, bool CPLX, int NT, bool ADJ>
__global__ void __launch_bounds__(512) bsr_blk_mfma_kernel(const BsrArgs p, const int *__restrict__ ent,
                                                           int yrow, int xrow, int nstrips, int kparts,
                                                           int vec_ok) {
    typedef typename BsrMfmaElem<RV, CPLX>::type EV; // the values
    typedef typename BsrMfmaElem<R, CPLX>::type E;   // the vectors
    typedef typename BsrMfma<R>::acc_t acc_t;
    typedef BlkVec<EV> VV;
    typedef BlkVec<E> V;
    constexpr int VA = 16 / (int)sizeof(EV), VE = 16 / (int)sizeof(E), H = VA / VE;
    constexpr int XW = NT * 16, NC = CPLX ? 2 : 1, U = 4;
    static_assert(VA == H * VE, "a group of VA k is H 16-byte pieces of x");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    E *xs = (E *)smem;
    const EV *__restrict__ v = (const EV *)p.v;
    const E *__restrict__ x = (const E *)p.x;
    E *__restrict__ y = (E *)p.y;
    const int bi = p.bi, bd = p.bd;
    const int nss = (bd + 4 * VA - 1) / (4 * VA), kpad = nss * 4 * VA; // k-steps of 4 VA
    const int xbuf = kpad * XW;                                        // elements per x buffer
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long i = blockIdx.x, col0 = (long)blockIdx.y * XW;
    const bool active = w < nstrips * kparts;
    const int strip = w % nstrips, kp = w / nstrips;
    const int ar = lane & 15, kq = lane >> 4;
    const int arow = strip * 16 + ar;
    const bool arow_ok = active && arow < bi;

    // staging order: element e = outer * nin + inner, inner the fastest index of x (the rhs
    // column for row-major x, else the domain row), walked by steps of the workgroup size
    const int nin = xrow ? XW : kpad, nout = xrow ? kpad : XW;
    const int in0 = tid % nin, out0 = tid / nin, din = nthr % nin, dout = nthr / nin;
    auto stage = [&](int j, int buf) {
        const int dj = p.jj[j];
        if (dj < 0) return;
        E *dst = xs + buf * xbuf;
        int in = in0, out = out0;
        while (out < nout) {
            E t[4];
            int kk[4], cc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                kk[q] = xrow ? out : in;
                cc[q] = xrow ? in : out;
                const long col = col0 + cc[q];
                t[q] = E{};
                if (out < nout && kk[q] < bd && col < p.ncols)
                    t[q] = xrow ? x[(long)(dj + kk[q]) * p.ldx + col] : x[(long)(dj + kk[q]) + col * p.ldx];
                if (out >= nout) kk[q] = -1;
                in += din;
                out += dout;
                if (in >= nin) {
                    in -= nin;
                    ++out;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (kk[q] >= 0) dst[((kk[q] / VE) * XW + cc[q]) * VE + (kk[q] % VE)] = t[q];
        }
    };
    // (ADJ conjugates in the element loads' own expressions: written as statements after the
    // loads, the complex<double> adjoint compiles differently, profiles/bsr_kernels_refactor_isa.txt)
    auto load_a = [&](const EV *vb, int ss) {
        VV a;
#pragma unroll
        for (int t = 0; t < VA; ++t) a.e[t] = EV{};
        const int k0 = (ss * 4 + kq) * VA;
        if (arow_ok && k0 < bd) {
            if (!p.block_im_fast) {
                const EV *src = vb + (long)arow * bd + k0;
                if (vec_ok && k0 + VA <= bd) {
                    a = *(const VV *)src;
                    if constexpr (ADJ) {
#pragma unroll
                        for (int t = 0; t < VA; ++t) a.e[t] = Ops<EV>::conj(a.e[t]);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < VA; ++t)
                        if (k0 + t < bd) {
                            if constexpr (ADJ) a.e[t] = Ops<EV>::conj(src[t]);
                            else a.e[t] = src[t];
                        }
                }
            } else {
#pragma unroll
                for (int t = 0; t < VA; ++t)
                    if (k0 + t < bd) {
                        if constexpr (ADJ) a.e[t] = Ops<EV>::conj(vb[arow + (long)(k0 + t) * bi]);
                        else a.e[t] = vb[arow + (long)(k0 + t) * bi];
                    }
            }
        }
        return a;
    };
    acc_t accR[NT], accI[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) accR[nt] = accI[nt] = acc_t{0, 0, 0, 0};
    auto apply = [&](const VV &af, int ss, const E *xb) {
        E a[VA]; // (the mixed product's up-conversion: exact)
#pragma unroll
        for (int t = 0; t < VA; ++t) a[t] = to_vec<E>(af.e[t]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const V b = *(const V *)(xb + (((ss * 4 + kq) * H + h) * XW + nt * 16 + ar) * VE);
#pragma unroll
                for (int u = 0; u < VE; ++u) {
                    const E ak = a[h * VE + u];
                    if constexpr (CPLX) {
                        accR[nt] = BsrMfma<R>::mma(ak.x, b.e[u].x, accR[nt]);
                        accI[nt] = BsrMfma<R>::mma(ak.x, b.e[u].y, accI[nt]);
                        accR[nt] = BsrMfma<R>::mma(-ak.y, b.e[u].y, accR[nt]);
                        accI[nt] = BsrMfma<R>::mma(ak.y, b.e[u].x, accI[nt]);
                    } else {
                        accR[nt] = BsrMfma<R>::mma(ak, b.e[u], accR[nt]);
                    }
                }
            }
        }
    };

    const int jb = p.ii[i], je = p.ii[i + 1];
    if (jb < je) stage(jb, 0);
    __syncthreads();
    for (int j = jb; j < je; ++j) {
        const int buf = (j - jb) & 1;
        const bool on = active && p.jj[j] >= 0; // wave-uniform: the MFMAs run with all 64 lanes
        const EV *vb = v + (long)(ADJ ? ent[j] : j) * bi * bd; // (wave-uniform)
        const E *xb = xs + buf * xbuf;
        // the block's first U fragments are in flight while the next x block is staged
        VV a[U];
        if (on) {
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = load_a(vb, kp + u * kparts);
        }
        if (j + 1 < je) stage(j + 1, buf ^ 1);
        if (on) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (kp + u * kparts < nss) apply(a[u], kp + u * kparts, xb);
            for (int ss = kp + U * kparts; ss < nss; ss += U * kparts) {
#pragma unroll
                for (int u = 0; u < U; ++u) a[u] = load_a(vb, ss + u * kparts);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (ss + u * kparts < nss) apply(a[u], ss + u * kparts, xb);
            }
        }
        __syncthreads(); // buffer buf is free again, buffer buf ^ 1 is complete
    }
    if (kparts > 1) {
        // the x buffers are dead (every path above ends in a barrier): partial tiles of the
        // k-parts 1.. to LDS, summed by part 0 in part order
        R *red = (R *)smem;
        if (active && kp > 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    red[(((w * NT + nt) * NC + 0) * 4 + q) * 64 + lane] = accR[nt][q];
                    if constexpr (CPLX) red[(((w * NT + nt) * NC + 1) * 4 + q) * 64 + lane] = accI[nt][q];
                }
        }
        __syncthreads();
        if (active && kp == 0) {
            for (int k2 = 1; k2 < kparts; ++k2) {
                const int w2 = strip + k2 * nstrips;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        accR[nt][q] += red[(((w2 * NT + nt) * NC + 0) * 4 + q) * 64 + lane];
                        if constexpr (CPLX) accI[nt][q] += red[(((w2 * NT + nt) * NC + 1) * 4 + q) * 64 + lane];
                    }
            }
        }
    }
    if (!active || kp != 0) return;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = strip * 16 + BsrMfma<R>::row(lane, q);
            const long col = col0 + nt * 16 + ar;
            if (row >= bi || col >= p.ncols) continue;
            const long img = i * bi + row;
            E *yp = yrow ? y + img * p.ldy + col : y + img + col * p.ldy;
            E out;
            if constexpr (CPLX)
                out = Ops<E>::scale(E{accR[nt][q], accI[nt][q]}, p.alpha_re, p.alpha_im);
            else
                out = Ops<E>::scale(accR[nt][q], p.alpha_re, p.alpha_im);
            *yp = p.add ? Ops<E>::add(*yp, out) : out;
        }
}

/// false: not this shape (the generic kernel runs).  Values RV, vectors R (the same, or float
/// values and double vectors, or half values and float vectors: form 16).  Limits, by the
/// vector type: bi <= 128 (8 strips, one wave each), two x buffers of kpad x 16 columns within 64 KB of LDS (kpad: bd rounded up to 4 VA; bd
/// <= 128 for complex<double>, 256 for 8-byte and 512 for 4-byte vector elements), NT reduced to
/// stay within 32 KB where possible, at most 65535 groups of NT column tiles.
/// ent: the in-place adjoint (form 17; same-type products), under the same limits.
template <typename RV, typename R, bool CPLX>
bool launch_bsr_blk_mfma(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s, const int *ent) {
    typedef typename BsrMfmaElem<RV, CPLX>::type EV;
    typedef typename BsrMfmaElem<R, CPLX>::type E;
    constexpr bool SAME = std::is_same<RV, R>::value;
    constexpr int ES = (int)sizeof(E), VA = 16 / (int)sizeof(EV);
    if (ent && !SAME) return false; // the mixed in-place adjoint is not instantiated
    const int nstrips = (a.bi + 15) / 16;
    if (nstrips > 8 || a.block_rows >= (1L << 31)) return false;
    const int nss = (a.bd + 4 * VA - 1) / (4 * VA), kpad = nss * 4 * VA;
    const int kparts = std::min(nstrips == 1 ? 4 : nstrips == 2 ? 2 : 1, nss);
    const int nw = nstrips * kparts;
    auto lds_of = [&](int nt) {
        const long xb = 2L * kpad * nt * 16 * ES;
        const long red = kparts > 1 ? (long)nw * nt * (CPLX ? 2 : 1) * 4 * 64 * (long)sizeof(R) : 0;
        return std::max(xb, red);
    };
    // NT column tiles share the value fragments; within 32 KB of LDS where that keeps NT > 1
    // (several workgroups per CU hide the value stream's latency)
    int nt = a.ncols <= 16 ? 1 : a.ncols <= 32 ? 2 : 4;
    while (nt > 1 && lds_of(nt) > 32768) nt /= 2;
    const long lds = lds_of(nt);
    if (lds > 65536) return false;
    const long ngroups = (a.ncols + nt * 16 - 1) / (nt * 16);
    if (ngroups > 65535) return false;
    const int vec_ok = ((long)a.bd * (long)sizeof(EV)) % 16 == 0 && ((size_t)a.v & 15) == 0 ? 1 : 0;
    g_bsr_tune.last = ent ? 17 : SAME ? 14 : 16;
    KernelTimer timer("bsr", s);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)a.block_rows, (unsigned)ngroups), dim3(64 * nw), lds, s, a,
                           ent, yrow ? 1 : 0, xrow ? 1 : 0, nstrips, kparts, vec_ok);
    };
    auto go_nt = [&](auto adj) {
        constexpr bool ADJ = SAME && decltype(adj)::value; // (the only adjoints instantiated)
        if (nt == 1) go(bsr_blk_mfma_kernel<RV, R, CPLX, 1, ADJ>);
        else if (nt == 2) go(bsr_blk_mfma_kernel<RV, R, CPLX, 2, ADJ>);
        else go(bsr_blk_mfma_kernel<RV, R, CPLX, 4, ADJ>);
    };
    if (ent) go_nt(std::true_type{});
    else go_nt(std::false_type{});
    SBX_HIP_CHECK(hipGetLastError());
    return true;
}

/// launch_bsr_blk_mfma by element types: values EV, vectors EX
template <typename EV, typename EX = EV>
bool launch_blk(const BsrArgs &a, bool yrow, bool xrow, hipStream_t s, const int *ent = nullptr) {
    static_assert(BsrMfmaScalar<EV>::cplx == BsrMfmaScalar<EX>::cplx, "both real or both complex");
    return launch_bsr_blk_mfma<typename BsrMfmaScalar<EV>::real, typename BsrMfmaScalar<EX>::real,
                               BsrMfmaScalar<EX>::cplx>(a, yrow, xrow, s, ent);
}

/// A mixed product (values EV, vectors EX).  The matrix-core form takes dense blocks from
/// blk_min x blk_min on (blk_mfma, blk_min and variant as for bsr_blk_mfma_kernel) where it was
/// measured faster than the generic mixed form by more than the larger round-to-round spread of
/// the two (8^4 9-point operators, complex<float> values, complex<double> vectors,
/// profiles/bsr_mixed_measure.txt): 32x32 blocks and larger at any column count (1.25-5.8x), 16x16
/// and 24x24 from 4 columns (1.04x / 1.02x at 4, 2.6-4.0x from 12; at one column 0.73x / 0.89x);
/// between the measured sizes the bound goes by the block's elements: 1024 and more at any column
/// count, fewer from 4 columns (float -> double: the same bound, not measured).
/// Half-precision operators with single-precision vectors, measured the same way (complex32
/// values, complex<float> vectors, profiles/bsr_half_measure.txt): 32x32 blocks and larger at any
/// column count (1.66-8.6x), 16x16 from 4 columns (1.38x at 4, 3.3-4.3x from 12; at one column
/// 0.93x), 24x24 from 12 columns (2.3-3.9x; 0.79x / 0.87x at 1 / 4 columns: its rows are padded to
/// the k-step of 16, the work of a 32x32 block); between the measured sizes by the block's
/// elements, more than 256 and fewer than 1024 from 12 columns (float16 -> float: the same
/// bound, carried over, not measured).
/// blk_mfma 2: no column bound.
/// 12x12 blocks (the lattice's fine operator) from mixed12_min_cols rhs columns on take the
/// choices of launch_bsr_mfma with the values read in EV: the LDS-DMA form (7, or 8 with packed
/// slots, mixed12_pack; variant 0, 9 blocks per row, row-major x with ldx == ncols <= 16, blk_pd
/// blocks ahead, values and x 16-byte aligned), the fragment gathers (10; 9 blocks per row) or the
/// generic rows (11; variant 1, any pattern); gemm.m3 does not apply (always 4 multiplications).
/// Measured against the generic mixed form (16^4 and 16^3 x 64 9-point operators, complex32 ->
/// complex<float> and complex<float> -> complex<double>, profiles/bsr_mixed12_measure.txt): faster
/// at every column count, 1.6-2.4x at 1 and 4 columns, 3.7-7.1x from 12, far beyond the spreads.
/// The default bound of 4 columns is a condition (tests pin 12x12 at 3 columns on the generic
/// form), not a crossover.  Against the same values widened on the same-type kernels the time
/// does not follow the bytes: 0.89-1.23x (see the profile).
/// 3x3 blocks and everything else run the generic mixed form.
template <typename EV, typename EX>
void launch_mixed(const BsrArgs &a, int nnz_per_row, bool yrow, bool xrow, hipStream_t s) {
    constexpr bool HALF = std::is_same<EV, f16>::value || std::is_same<EV, f16x2>::value;
    if (g_bsr_tune.mixed && a.bi == 12 && a.bd == 12 && a.ncols >= g_bsr_tune.mixed12_min_cols)
        return launch_bsr_mfma<typename BsrMfmaScalar<EV>::real, typename BsrMfmaScalar<EX>::real,
                               BsrMfmaScalar<EX>::cplx, 12, 12>(a, nnz_per_row, yrow, xrow, s);
    const long be = (long)a.bi * a.bd;
    const int min_cols = g_bsr_tune.blk_mfma >= 2 || be >= 32 * 32 ? 1 : HALF && be > 16 * 16 ? 12 : 4;
    if (g_bsr_tune.mixed && g_bsr_tune.blk_mfma && g_bsr_tune.variant != 1 && a.bi >= g_bsr_tune.blk_min &&
        a.bd >= g_bsr_tune.blk_min && a.ncols >= min_cols &&
        launch_blk<EV, EX>(a, yrow, xrow, s))
        return;
    launch_generic<EV, EX, 0, 0>(a, yrow, xrow, s);
}

/// Whether launch_typed's dense-block clause takes these blocks at this column count
/// (bsr.blk_mfma, bsr.blk_min, bsr.variant and the measured column thresholds, see launch_typed)
inline bool blk_mfma_admits(const BsrArgs &a) {
    return g_bsr_tune.blk_mfma && g_bsr_tune.variant != 1 && a.bi >= g_bsr_tune.blk_min &&
           a.bd >= g_bsr_tune.blk_min &&
           a.ncols >= (g_bsr_tune.blk_mfma >= 2 || a.bi * a.bd >= 32 * 32 ? 1 : a.bi * a.bd >= 24 * 24 ? 4 : 12);
}

template <typename E>
void launch_typed(const BsrArgs &a, int nnz_per_row, bool yrow, bool xrow, hipStream_t s) {
    const bool ell = nnz_per_row > 0 &&
                     (long)nnz_per_row * (a.bi * a.bd * (long)sizeof(E) + 4) <= ELL_LDS_BYTES;
    if (ell && a.bi == 3 && a.bd == 3)
        launch_ell<E, 3, 3>(a, nnz_per_row, yrow, xrow, s);
    else if (a.bi == 3 && a.bd == 3)
        launch_generic<E, E, 3, 3>(a, yrow, xrow, s);
    else if (a.bi == 12 && a.bd == 12)
        // one block row per wave: interleaving 2 or 4 rows per wave measured 6 % / 25 % slower
        // (more VGPRs, fewer waves to hide the HBM latency of the value stream)
        launch_bsr_mfma<typename BsrMfmaScalar<E>::real, typename BsrMfmaScalar<E>::real, BsrMfmaScalar<E>::cplx, 12, 12>(
            a, nnz_per_row, yrow, xrow, s);
    // dense blocks from blk_min x blk_min on: bsr_blk_mfma_kernel where it was measured faster
    // than the generic kernel by more than the round-to-round spread (8^4 9-point operators,
    // complex<float> and complex<double>, profiles/bsr_blocks_measure.txt): 32x32 blocks and
    // larger at any column count (1.15-8.7x), 24x24 from 4 columns (complex<double> n = 1: a
    // tie), 16x16 from 12 columns (complex<double> n = 1 / 4: 0.75x / 0.93x); between the
    // measured sizes the bound goes by the block's elements.  blk_mfma 2: no column bound
    else if (blk_mfma_admits(a) && launch_blk<E>(a, yrow, xrow, s))
        return;
    else
        launch_generic<E, E, 0, 0>(a, yrow, xrow, s);
}

/// The in-place adjoint of a plain operator: the matrix-core form where launch_typed's
/// dense-block clause would take the copy (same-type products; not 3x3 and 12x12 blocks, whose
/// LDS-DMA kernels stream contiguous value runs that an indirection breaks), else the generic form.
template <typename EV, typename EX>
void launch_adj(const BsrArgs &a, const int *ent, bool yrow, bool xrow, hipStream_t s) {
    if constexpr (std::is_same<EV, EX>::value) {
        if (!(a.bi == 3 && a.bd == 3) && !(a.bi == 12 && a.bd == 12) && blk_mfma_admits(a) &&
            launch_blk<EX>(a, yrow, xrow, s, ent))
            return;
    }
    g_bsr_tune.last = 18;
    launch_generic<EV, EX, 0, 0, true>(a, yrow, xrow, s, ent);
}

template <typename E>
__global__ void __launch_bounds__(256) gather_blocks_kernel(const E *__restrict__ src,
                                                            const int *__restrict__ perm,
                                                            long nblocks, long be, int conj,
                                                            E *__restrict__ dst) {
    const long total = nblocks * be;
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256L) {
        const long q = idx / be, e = idx - q * be;
        const E v = src[(long)perm[q] * be + e];
        dst[idx] = conj ? Ops<E>::conj(v) : v;
    }
}

template <typename E>
void gather_typed(const void *src, const int *perm, long nblocks, long be, bool cj, void *dst,
                  hipStream_t s) {
    const long blocks = std::min((nblocks * be + 255) / 256, 65536L);
    hipLaunchKernelGGL(gather_blocks_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, s,
                       (const E *)src, perm, nblocks, be, cj ? 1 : 0, (E *)dst);
    SBX_HIP_CHECK(hipGetLastError());
}

} // namespace

void launch_gather_blocks(int t, const void *src, const int *perm, long nblocks, long block_elems,
                          bool conj_values, void *dst, int device) {
    if (nblocks == 0 || block_elems == 0) return;
    set_device(device);
    hipStream_t s = get_stream(device);
    switch (t) {
    case SBX_CDOUBLE: return gather_typed<double2>(src, perm, nblocks, block_elems, conj_values, dst, s);
    case SBX_CFLOAT: return gather_typed<float2>(src, perm, nblocks, block_elems, conj_values, dst, s);
    case SBX_DOUBLE: return gather_typed<double>(src, perm, nblocks, block_elems, false, dst, s);
    case SBX_FLOAT: return gather_typed<float>(src, perm, nblocks, block_elems, false, dst, s);
    // half-precision operators: the copy stays in the operator's type (conjugation: a sign bit)
    case SBX_CHALF: return gather_typed<f16x2>(src, perm, nblocks, block_elems, conj_values, dst, s);
    case SBX_HALF: return gather_typed<f16>(src, perm, nblocks, block_elems, false, dst, s);
    default: throw Error("bsr: unsupported type");
    }
}

void launch_bsr(const BsrDesc &d, int device) {
    if (d.block_rows == 0 || d.ncols == 0) return;
    g_bsr_tune.last = 0;
    set_device(device);
    hipStream_t s = get_stream(device);
    BsrArgs a{};
    a.block_rows = d.block_rows;
    a.bi = d.bi;
    a.bd = d.bd;
    a.ii = d.ii;
    a.jj = d.jj;
    a.v = d.v;
    a.block_im_fast = d.block_im_fast ? 1 : 0;
    a.x = d.x;
    a.ldx = d.ldx;
    a.x_rows = d.x_rows;
    a.y = d.y;
    a.ldy = d.ldy;
    a.ncols = d.ncols;
    a.alpha_re = d.alpha.re;
    a.alpha_im = d.alpha.im;
    a.add = d.add ? 1 : 0;
    a.ilv = 2; // an XCD's row chunks visited as two interleaved halves (bsr_ell9_kernel)
    a.nt = g_bsr_tune.nt;
    a.tiles[0] = d.tiles[0];
    a.tiles[1] = d.tiles[1];
    if (d.adj_ent) {
        // the adjoint of a plain operator on A's own values (bsr.adj_inplace)
        const bool yr = d.y_row_major, xr = d.x_row_major;
        if (d.tv == SBX_CFLOAT && d.t == SBX_CDOUBLE) return launch_adj<float2, double2>(a, d.adj_ent, yr, xr, s);
        if (d.tv == SBX_FLOAT && d.t == SBX_DOUBLE) return launch_adj<float, double>(a, d.adj_ent, yr, xr, s);
        if (d.tv == SBX_CHALF && d.t == SBX_CFLOAT) return launch_adj<f16x2, float2>(a, d.adj_ent, yr, xr, s);
        if (d.tv == SBX_HALF && d.t == SBX_FLOAT) return launch_adj<f16, float>(a, d.adj_ent, yr, xr, s);
        if (d.tv != d.t) throw Error("bsr: unsupported pair of value and vector types");
        switch (d.t) {
        case SBX_CDOUBLE: return launch_adj<double2, double2>(a, d.adj_ent, yr, xr, s);
        case SBX_CFLOAT: return launch_adj<float2, float2>(a, d.adj_ent, yr, xr, s);
        case SBX_DOUBLE: return launch_adj<double, double>(a, d.adj_ent, yr, xr, s);
        case SBX_FLOAT: return launch_adj<float, float>(a, d.adj_ent, yr, xr, s);
        default: throw Error("bsr: unsupported type");
        }
    }
    if (d.tv != d.t) {
        // single-precision values with double-precision vectors, half-precision values with
        // single-precision vectors (bsr_krylov admits these four pairs)
        if (d.tv == SBX_CFLOAT && d.t == SBX_CDOUBLE)
            return launch_mixed<float2, double2>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
        if (d.tv == SBX_FLOAT && d.t == SBX_DOUBLE)
            return launch_mixed<float, double>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
        if (d.tv == SBX_CHALF && d.t == SBX_CFLOAT)
            return launch_mixed<f16x2, float2>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
        if (d.tv == SBX_HALF && d.t == SBX_FLOAT)
            return launch_mixed<f16, float>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
        throw Error("bsr: unsupported pair of value and vector types");
    }
    switch (d.t) {
    case SBX_CDOUBLE: return launch_typed<double2>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
    case SBX_CFLOAT: return launch_typed<float2>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
    case SBX_DOUBLE: return launch_typed<double>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
    case SBX_FLOAT: return launch_typed<float>(a, d.num_nnz_per_row, d.y_row_major, d.x_row_major, s);
    default: throw Error("bsr: unsupported type");
    }
}

} // namespace sbx
