"""Hermitian / symmetric output mode of the batched GEMM (sbx_tune_set "gemm.herm", off by
default): a tensor contracted with itself (one buffer passed as both operands, m == n) computes
only the upper triangle of 16x16 sub-tiles (gemm_wave_kernel) or of tiles (gemm_dma_kernel) and
stores each accumulator, conjugated for a Hermitian output, at its mirrored position too.

What is pinned, for C(i, j) with i the row (M) and j the column (N) index:
 * the read-back "gemm.last_herm": the tiles per batch entry the launch mirrored (0 = full product);
 * i <= j: the same values as the full product (herm 0) -- the same MFMA sequence, k partition and
   sums;
 * i > j: the value of the full product (diagonal tiles are computed whole) or the exact mirror
   of C(j, i); for complex types some elements must take the mirror branch and differ from the
   full product (whose imaginary part adds the same two products per k-step in the other order),
   else the test could not tell the feature from a full product;
 * float64: the full product's values everywhere (the products commute, the order is the same);
 * the oracle, with alpha = 1, beta = 0 and with complex alpha and beta on a random C (the mirror
   acts on the accumulator, before alpha and beta);
 * two herm 1 calls in a row give the same values (gemm.t48 17: the fused counters return to 0).

Two groups of the one-tile cases do not reach gemm_wave_kernel, by the library's dispatch, and are
full products, last_herm 0, pinned as such: complex128 (launch_tiled sends complex<double> to the
64x64 LDS-DMA tiles, one tile per batch entry here, and nothing is skipped inside a diagonal
tile), and complex64 with k <= 64 (launch_frag takes a short output dimension of up to 48
against a k of up to 64 for complex<float>: the fragment kernel)."""
import functools

import numpy as np
import pytest

from _common import oracle_contraction, oracle_gemm, random_valued, rel_err

pytestmark = pytest.mark.gpu

# the table of tests/test_gpu_gemm.py
TOL = {np.complex128: 1e-10, np.float64: 1e-10, np.complex64: 1e-5, np.float32: 1e-5}
KEYS = ("gemm.herm", "gemm.t48", "gemm.m3", "gemm.share_ab")


def _cplx(dtype):
    return np.dtype(dtype).kind == "c"


def _ops(dtype, major, tb="C"):
    """(ta, tb, lda) of A op(A) with one buffer: M-major 'N', tb; K-major 'C' / 'T', 'N'"""
    if not _cplx(dtype) and tb == "C":
        tb = "T"
    return ("N", tb) if major == "M" else (tb, "N")


@functools.lru_cache(maxsize=None)
def _data(dtype, m, k, batch):
    a = random_valued(k * m * batch, dtype, 21)
    a.setflags(write=False)
    c0 = random_valued(m * m * batch, dtype, 22)
    c0.setflags(write=False)
    return a, c0


@functools.lru_cache(maxsize=None)
def _oracle(dtype, major, tb, m, k, batch):
    """A op(A) by the oracle (alpha = 1, beta = 0), computed once per case and left unchanged"""
    a, _ = _data(dtype, m, k, batch)
    ta, tb_ = _ops(dtype, major, tb)
    ld = m if major == "M" else k
    ref = np.zeros(m * m * batch, dtype)
    oracle_gemm(ta, tb_, m, m, k, 1.0, a, ld, k * m, a, ld, k * m, 0.0, ref, m, m * m, batch)
    ref.setflags(write=False)
    return ref


def _gemm(gpu, dtype, major, tb, m, k, batch, alpha=1.0, beta=0.0):
    """C = alpha A op(A) + beta C0 on the GPU with one buffer as both operands; C as [b, i, j]"""
    import torch
    import superbblas_amd as sb
    a, c0 = _data(dtype, m, k, batch)
    ta, tb_ = _ops(dtype, major, tb)
    ld = m if major == "M" else k
    t_a = torch.from_numpy(a.copy()).to(gpu)
    t_c = torch.from_numpy(c0.copy()).to(gpu)
    sb.xgemm_batch_strided(ta, tb_, m, m, k, alpha, t_a, ld, k * m, t_a, ld, k * m, beta, t_c, m,
                           m * m, batch)
    torch.cuda.synchronize()
    # column-major m x m per batch entry: [b, j, i] -> [b, i, j]
    return (t_c.cpu().numpy().reshape(batch, m, m).transpose(0, 2, 1),
            sb.tune_get("gemm.last_herm"))


def _mirror(c, conj):
    ct = c.transpose(0, 2, 1)
    return np.conj(ct) if conj else ct


def _check_bits(out0, out1, conj, dtype, full):
    """checks 2-5 of the module docstring; `full`: the launch is a full product"""
    m = out0.shape[1]
    upper = np.triu(np.ones((m, m), bool))[None]
    lower = ~upper
    same = out1 == out0
    assert np.all(same | lower), "computed elements (i <= j) differ from the full product"
    mirrored = out1 == _mirror(out1, conj)
    assert np.all(same | mirrored | upper), "i > j: neither the full product nor the mirror"
    took_mirror = int(np.count_nonzero(lower & mirrored & ~same))
    print("elements mirrored and different from the full product: %d of %d below the diagonal"
          % (took_mirror, int(np.count_nonzero(np.broadcast_to(lower, out0.shape)))))
    if full or not _cplx(dtype):
        assert np.array_equal(out1, out0)
    else:
        assert took_mirror > 0


def _case(gpu, dtype, major, tb, m, k, batch, expect, tunes=()):
    import superbblas_amd as sb
    old = {key: sb.tune_get(key) for key in KEYS}
    cplx = _cplx(dtype)
    conj = cplx and tb == "C"
    alpha, beta = (0.5 - 0.5j, 0.25 + 1j) if cplx else (0.5, 0.25)
    try:
        for key, v in tunes:
            sb.tune_set(key, v)
        sb.tune_set("gemm.herm", 0)
        out0, lh0 = _gemm(gpu, dtype, major, tb, m, k, batch)
        sb.tune_set("gemm.herm", 1)
        out1, lh1 = _gemm(gpu, dtype, major, tb, m, k, batch)
        out1b, _ = _gemm(gpu, dtype, major, tb, m, k, batch)
        out2, lh2 = _gemm(gpu, dtype, major, tb, m, k, batch, alpha, beta)
    finally:
        for key, v in old.items():
            sb.tune_set(key, v)
    print("last_herm: herm 0 %d, herm 1 %d" % (lh0, lh1))
    assert lh0 == 0
    assert lh1 == expect and lh2 == expect
    _check_bits(out0, out1, conj, dtype, full=expect == 0)
    assert np.array_equal(out1b, out1)
    ref = _oracle(dtype, major, tb, m, k, batch).reshape(batch, m, m).transpose(0, 2, 1)
    _, c0 = _data(dtype, m, k, batch)
    c0 = c0.reshape(batch, m, m).transpose(0, 2, 1)
    e1, e2 = rel_err(out1, ref), rel_err(out2, alpha * ref.astype(np.complex128) + beta * c0)
    print("rel err vs the oracle: %.3g (alpha 1, beta 0), %.3g (alpha, beta)" % (e1, e2))
    assert e1 < TOL[dtype]
    assert e2 < TOL[dtype]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64])
@pytest.mark.parametrize("m,k,batch", [(48, 3072, 3), (40, 1000, 2), (36, 24, 1)])
@pytest.mark.parametrize("tb", ["C", "T"])
@pytest.mark.parametrize("t48", [5, 17])
def test_herm_wave(gpu, dtype, m, k, batch, tb, t48):
    """'N', tb on one M-major buffer, one tile per batch entry (the chain's y^H y shape): the
    wave-ring kernel skips its 3 sub-tiles below the diagonal -- several splits with the tree
    sum, ragged m and k, a k shorter than one slab ring; tb 'T' on a complex type is the plain
    (symmetric) mirror.  complex128 runs on the 64x64 LDS-DMA tile and complex64 with k = 24 on
    the fragment kernel instead: full products."""
    expect = 0 if dtype is np.complex128 or (dtype is np.complex64 and k <= 64) else 3
    _case(gpu, dtype, "M", tb, m, k, batch, expect, tunes=(("gemm.t48", t48),))


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64])
@pytest.mark.parametrize("major", ["K", "M"])
@pytest.mark.parametrize("m,k,batch,expect", [(256, 1536, 3, 1), (300, 200, 2, 3),
                                              (130, 520, 1, 1), (96, 512, 2, 1)])
def test_herm_dma(gpu, dtype, major, m, k, batch, expect):
    """('C','N') on a K-major and ('N','C') on an M-major buffer with several tiles: 2 x 2 tiles
    of 128, 3 x 3 with a ragged edge, a 2-row last tile, 2 x 2 tiles of 64; the grid holds the
    tiles with ti <= tj, the others are mirrored (tm (tm - 1) / 2 of them)"""
    _case(gpu, dtype, major, "C", m, k, batch, expect)


def test_herm_dma_symmetric_and_unshared(gpu):
    """the plain mirror of a complex symmetric product A^T A, and gemm.herm without
    gemm.share_ab (the mode does not depend on the shared slab image)"""
    _case(gpu, np.complex64, "K", "T", 130, 520, 2, 1)
    _case(gpu, np.complex128, "M", "C", 130, 72, 2, 1, tunes=(("gemm.share_ab", 0),))


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_herm_fallbacks(gpu, dtype):
    """launches outside the two kernels stay full products and report 0: the fragment kernel
    (m = 24) and the 3-multiplication form (gemm.m3 1) at m = 256"""
    _case(gpu, dtype, "M", "C", 24, 512, 2, 0)
    _case(gpu, dtype, "K", "C", 256, 512, 1, 0, tunes=(("gemm.m3", 1),))


def test_herm_different_operands(gpu):
    """two different buffers of the same shape: a full product"""
    import torch
    import superbblas_amd as sb
    m, k, batch = 130, 72, 2
    a = random_valued(k * m * batch, np.complex64, 31)
    b = random_valued(k * m * batch, np.complex64, 32)
    ref = np.zeros(m * m * batch, np.complex64)
    oracle_gemm("C", "N", m, m, k, 1.0, a, k, k * m, b, k, k * m, 0.0, ref, m, m * m, batch)
    t_a, t_b = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    t_c = torch.zeros(m * m * batch, dtype=torch.complex64, device=gpu)
    old = sb.tune_get("gemm.herm")
    sb.tune_set("gemm.herm", 1)
    try:
        sb.xgemm_batch_strided("C", "N", m, m, k, 1.0, t_a, k, k * m, t_b, k, k * m, 0.0, t_c, m,
                               m * m, batch)
        torch.cuda.synchronize()
        assert sb.tune_get("gemm.last_herm") == 0
    finally:
        sb.tune_set("gemm.herm", old)
    assert rel_err(t_c.cpu().numpy(), ref) < TOL[np.complex64]


def test_herm_chain_contraction(gpu):
    """step (3) of tests/test_gpu_chain.py::test_chain_reduced with n = 12 columns, so that the
    TSnsN blocks are the chain's 48 x 48: sb.contraction hands the tensor's pointer and strides to
    the GEMM for both operands (read back: 3 sub-tiles mirrored per block).  Rows of a block are
    the first operand's (S, n), columns the second's (s, N)."""
    import torch
    import superbblas_amd as sb
    Ls, Lt, ncols, s_, c_ = 4, 8, 12, 4, 3
    dx = [1, Ls, Ls, Ls, Lt, s_, c_, ncols]
    dr = [Lt, s_, ncols, s_, ncols]
    cf = np.complex64
    y = random_valued(int(np.prod(dx)), cf, 41)
    t_y = torch.from_numpy(y).to(gpu)
    p_x = [([0] * 8, dx)]
    outs, lh = [], []
    old = sb.tune_get("gemm.herm")
    try:
        for herm in (0, 1):
            sb.tune_set("gemm.herm", herm)
            t_r = torch.empty(int(np.prod(dr)), dtype=torch.complex64, device=gpu)
            sb.contraction(1.0, p_x, [0] * 8, dx, dx, "pXYZTSCn", True, [t_y], p_x, [0] * 8, dx,
                           dx, "pXYZTsCN", False, [t_y], 0.0, [([0] * 5, dr)], [0] * 5, dr, dr,
                           "TSnsN", [t_r])
            torch.cuda.synchronize()
            lh.append(sb.tune_get("gemm.last_herm"))
            outs.append(t_r.cpu().numpy().reshape(Lt, s_ * ncols, s_ * ncols))
    finally:
        sb.tune_set("gemm.herm", old)
    assert lh == [0, 3]
    _check_bits(outs[0], outs[1], True, cf, full=False)
    r_ref = np.zeros(int(np.prod(dr)), cf)
    oracle_contraction(1.0, "pXYZTSCn", [0] * 8, dx, dx, True, y, "pXYZTsCN", [0] * 8, dx, dx,
                       False, y, 0.0, "TSnsN", [0] * 5, dr, dr, r_ref)
    assert rel_err(outs[1], r_ref) < 2e-5
