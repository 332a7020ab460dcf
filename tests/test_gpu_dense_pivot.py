"""Dense batched solvers on matrices whose pivots leave the diagonal (kernels_dense.hip:
inv_wave_kernel / gj_step, gesv_wave_kernel, gesv_kernel, potrf_*), against a long-double
elimination (tests/_dense.py ld_solve / ld_inverse / ld_cholesky_upper).

Two input families.  perm_dominant: row-permuted diagonally dominant integer matrices, the pivot
sequence fixed by the permutation (matrix 0 swaps at every step but the last, matrix 1 never),
held to the project's dense tolerances (test_gpu_dense.py _tol, of the largest entry of the
truth).  rand_capped: uniform random matrices with cond_2 <= 1e3, held to
F * max(e_lapack, n eps): e_lapack the error of numpy's LAPACK in the same precision on the same
matrix against the same truth, F measured once (profiles/dense_pivot_measure.txt).

Every size of the wave kernels' compile-time variants (WNM 4 / 8 / 12 / 16, full and partial),
batches of two full workgroups and a ragged tail, the workgroup kernels on both sides of their
LDS limit (n = 64 / 65 for complex<double>)."""
import contextlib
import functools

import numpy as np
import pytest

from _dense import (from_matrices, ld_cholesky_upper, ld_inverse, ld_solve, perm_dominant,
                    rand_capped, to_matrices)
from _golden import gen

pytestmark = pytest.mark.gpu

TYPES = [np.complex128, np.float64, np.complex64, np.float32]
# (n, dense.wave); None: the default setting
SIZES = ([(n, 1) for n in (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16)] +
         [(n, 0) for n in (2, 7, 12, 16)] + [(n, None) for n in (17, 33, 64, 65)])
GESM_N = [2, 4, 7, 8, 12, 16, 17, 33]

# F of the rand_capped bound F * max(e_lapack, n eps), per operation and type: the next power of
# two at or above twice the worst ratio measured on an MI355X (profiles/dense_pivot_measure.txt,
# by tools/studies/dense_pivot_measure.py).  Worst ratios: inversion 2.03 / 9.03 / 5.75 / 26.7,
# gesm 2.20 / 7.54 / 3.56 / 27.1, cholesky 0.47 / 0.48 / 0.47 / 0.49.
#
# The three values above 16 are no loss of accuracy in a kernel (that file has the study): every worst matrix's
# error is 0.04 - 0.35 eps cond_2.  numpy's linalg computes single-precision input in double and
# rounds the result, so for float32 / complex64 e_lapack is 0.1 - 0.6 eps whatever the condition
# number and the bound is F n eps: float32's 26.7 and 27.1 are one 2 x 2 matrix of cond_2 738
# inverted to 53 eps = 0.07 eps cond_2 (28 eps by the workgroup kernel, which divides as getrs
# does).  float64's 9.03 is one 5 x 5 matrix of cond_2 757 with 45 eps = 0.06 eps cond_2 where
# LAPACK has 4.4 eps: the per-matrix ratio of two errors that are both far below eps cond_2 has a
# long tail either way -- over 4000 such matrices per size a float64 emulation of the kernel's
# order has a median ratio of 0.2 - 0.3 and a maximum of 11 - 25 against LAPACK, and LAPACK 7 - 19
# against the emulation.
_T = ("complex128", "float64", "complex64", "float32")
F = {"inversion": dict(zip(_T, (8, 32, 16, 64))),
     "gesm": dict(zip(_T, (8, 16, 8, 64))),
     "cholesky": dict(zip(_T, (1, 1, 1, 1)))}

# (operation, kernel path, type, n, the case's worst ratio, that matrix's error / eps, numpy's
# error / eps, cond_2): filled as the tests run, read by tools/studies/dense_pivot_measure.py
RATIOS = []


def _tol(t):
    """test_gpu_dense.py _tol"""
    return 1e-12 if np.dtype(t) in (np.float64, np.complex128) else 2e-5


def _k(n):
    """two full workgroups of the wave kernels (4 waves of 64 // n matrices) and a ragged tail"""
    return 2 * 4 * (64 // n) + 3 if n <= 16 else 3


def _ids(v):
    return v.__name__ if isinstance(v, type) else None


@contextlib.contextmanager
def _wave(w):
    import superbblas_amd as sb
    old = sb.tune_get("dense.wave")
    if w is not None:
        sb.tune_set("dense.wave", w)
    try:
        yield
    finally:
        sb.tune_set("dense.wave", old)


def _frozen(*xs):
    for x in xs:
        x.setflags(write=False)
    return xs


def _rel(out, truth):
    """per matrix: the largest error relative to the largest entry of the truth"""
    ax = tuple(range(1, truth.ndim))
    return (np.abs(out - truth).max(axis=ax) / np.abs(truth).max(axis=ax)).astype(np.float64)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _check(kind, op, path, dtype, a, err, e_lapack):
    """a: the matrices of the errors err, for their size and condition numbers"""
    n, name = a.shape[1], np.dtype(dtype).name
    if kind == "perm":
        print("%s %s %s n=%d: err %.3g (matrix 0, every step swaps: %.3g; tolerance %.3g)" % (
            op, path, name, n, err.max(), err[0], _tol(dtype)))
        assert err.max() < _tol(dtype), (int(err.argmax()), err.max())
        return
    eps = float(np.finfo(dtype).eps)
    ratio = err / np.maximum(e_lapack, n * eps)
    i = int(ratio.argmax())
    cond = float(np.linalg.cond(a[i].astype(np.complex128)))
    RATIOS.append((op, path, name, n, float(ratio[i]), err[i] / eps, e_lapack[i] / eps, cond))
    print("%s %s %s n=%d: worst ratio %.3g (F %g) at matrix %d: err %.3g eps, numpy %.3g eps, "
          "cond %.3g" % (op, path, name, n, ratio[i], F[op][name], i, err[i] / eps,
                         e_lapack[i] / eps, cond))
    assert ratio[i] <= F[op][name], (i, ratio[i])


def _path(n, wave):
    return "wave" if n <= 16 and wave != 0 else "workgroup"


def _full(dim):
    return [([0] * len(dim), list(dim))]


# ---- inversion ----

@functools.lru_cache(maxsize=None)
def _inv_case(kind, n, dtype):
    """the matrices, their long-double inverses and the error of numpy's inv in dtype"""
    a = perm_dominant(_k(n), n, dtype)[0] if kind == "perm" else rand_capped(_k(n), n, dtype)
    truth = ld_inverse(a)
    return _frozen(a, truth, _rel(np.linalg.inv(a), truth))


def _invert(gpu, a, layout):
    import torch
    import superbblas_amd as sb
    dim = list(a.shape)
    v = torch.from_numpy(from_matrices(a, layout, dim, "i", "j").copy()).to(gpu)
    sb.inversion(_full(dim), dim, layout, [v], "i", "j")
    torch.cuda.synchronize()
    return to_matrices(v.cpu().numpy(), layout, dim, "i", "j")


@pytest.mark.parametrize("dtype", TYPES, ids=_ids)
@pytest.mark.parametrize("n,wave", SIZES)
@pytest.mark.parametrize("kind,layout", [("perm", "tij"), ("perm", "tji"), ("rand", "tij")])
def test_inversion_pivots(gpu, kind, layout, n, wave, dtype):
    """"tij": the caller's row-major matrices, inverted in place when they are small; "tji":
    column-major, through a working copy"""
    a, truth, e_lapack = _inv_case(kind, n, dtype)
    with _wave(wave):
        out = _invert(gpu, a, layout)
    _check(kind, "inversion", _path(n, wave), dtype, a, _rel(out, truth), e_lapack)


# ---- gesm ----

def _alpha(dtype):
    return 0.5 - 1j if np.dtype(dtype).kind == "c" else 0.5


@functools.lru_cache(maxsize=None)
def _gesm_case(kind, n, m, dtype):
    """C [t, i, j], x [t, j, r], alpha C^-1 x [t, i, r] in long double and the error of
    alpha * numpy's solve in dtype"""
    k = _k(n)
    c = perm_dominant(k, n, dtype)[0] if kind == "perm" else rand_capped(k, n, dtype)
    x = gen("int" if kind == "perm" else "rand", k * n * m, 5, dtype).reshape(k, n, m)
    truth = _alpha(dtype) * ld_solve(c, x)
    same = (np.asarray(_alpha(dtype), dtype) * np.linalg.solve(c, x)).astype(dtype)
    return _frozen(c, x, truth, _rel(same, truth))


def _gesm(gpu, c, x, dtype, yl):
    """y (labels yl) = alpha C^-1 x with C "tij" and x "tjr"; returns y as [t, i, r]"""
    import torch
    import superbblas_amd as sb
    k, n, m = x.shape
    dims = {"t": k, "i": n, "r": m}
    dc, dx, dy = [k, n, n], [k, n, m], [dims[l] for l in yl]
    tc = torch.from_numpy(c.ravel().copy()).to(gpu)
    tx = torch.from_numpy(x.ravel().copy()).to(gpu)
    ty = torch.zeros(k * n * m, dtype=tx.dtype, device=gpu)
    sb.gesm(_alpha(dtype), _full(dc), dc, "tij", [tc], "i", "j", _full(dx), dx, "tjr", [tx],
            _full(dy), dy, yl, [ty])
    torch.cuda.synchronize()
    # C and x come back as they went in
    assert np.array_equal(_bits(tc.cpu().numpy()), _bits(c.ravel()))
    assert np.array_equal(_bits(tx.cpu().numpy()), _bits(x.ravel()))
    return ty.cpu().numpy().reshape(dy).transpose([yl.index(l) for l in "tir"])


@pytest.mark.parametrize("dtype", TYPES, ids=_ids)
@pytest.mark.parametrize("m", ["1", "n", "70"])
@pytest.mark.parametrize("n", GESM_N)
@pytest.mark.parametrize("kind", ["perm", "rand"])
def test_gesm_pivots(gpu, kind, n, m, dtype):
    """the three routes of dense_solve: straight between the caller's tensors (gesv_wave_kernel
    reading x and writing y in their own orientations, C factored in registers), through working
    copies where the LU is kept (y with the batch label last, which the direct path declines),
    and the workgroup-per-matrix kernel (dense.wave 0: piv[] applied to the right-hand sides);
    n > 16 takes the workgroup kernel on every route"""
    m = n if m == "n" else int(m)
    c, x, truth, e_lapack = _gesm_case(kind, n, m, dtype)
    for route, wave, yl in (("direct", None, "tri"), ("copies", None, "irt"), ("wave0", 0, "tri")):
        with _wave(wave):
            out = _gesm(gpu, c, x, dtype, yl)
        path = "%s m=%d" % (route if n <= 16 else "workgroup", m)
        _check(kind, "gesm", path, dtype, c, _rel(out, truth), e_lapack)


# ---- a singular matrix among good ones ----

def _singular_batch(n, dtype):
    a = rand_capped(35, n, dtype).copy()
    a[17, :, 5] = 0  # column 5 of matrix 17: the LU stops at pivot 6
    return a


@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=_ids)
def test_singular_neighbour(gpu, dtype):
    """dense.cpp dense_inversion, the in-place path: a singular matrix is left as it was and the
    other matrices of the batch hold their inverses when the error is thrown -- the infinities of
    the failed matrix's lanes reach none of its neighbours in the wave"""
    import torch
    import superbblas_amd as sb
    n = 12
    a = _singular_batch(n, dtype)
    dim = list(a.shape)
    good = np.arange(35) != 17
    truth = ld_inverse(a[good])
    e_lapack = _rel(np.linalg.inv(a[good]), truth)
    v = torch.from_numpy(a.ravel().copy()).to(gpu)
    with _wave(1):
        with pytest.raises(sb.SuperbblasError, match=r"lapack routine: 6(\D|$)"):
            sb.inversion(_full(dim), dim, "tij", [v], "i", "j")
        torch.cuda.synchronize()
    out = v.cpu().numpy().reshape(dim)
    assert np.array_equal(_bits(out[17]), _bits(a[17]))
    assert np.isfinite(out[good].view(np.finfo(dtype).dtype)).all()
    _check("rand", "inversion", "wave", dtype, a[good], _rel(out[good], truth), e_lapack)


@pytest.mark.parametrize("dtype", [np.complex128, np.float32], ids=_ids)
@pytest.mark.parametrize("n,wave", [(12, 0), (17, None)])
def test_singular_workgroup(gpu, n, wave, dtype):
    """the workgroup-per-matrix kernel: the error and its info"""
    import torch
    import superbblas_amd as sb
    a = _singular_batch(n, dtype)
    dim = list(a.shape)
    v = torch.from_numpy(a.ravel().copy()).to(gpu)
    with _wave(wave):
        with pytest.raises(sb.SuperbblasError, match=r"lapack routine: 6(\D|$)"):
            sb.inversion(_full(dim), dim, "tij", [v], "i", "j")
        torch.cuda.synchronize()


# ---- Cholesky ----

@functools.lru_cache(maxsize=None)
def _chol_case(n, dtype):
    """B^H B + I / 2 with B from rand_capped, exactly Hermitian in dtype; its upper factor in
    long double and the error of numpy's cholesky in dtype"""
    b = rand_capped(_k(n), n, dtype, seed=14).astype(np.complex128)
    h = np.einsum("tqr,tqc->trc", b.conj(), b)
    up = np.triu(h, 1)
    a = up + up.conj().transpose(0, 2, 1) + (np.triu(np.tril(h)).real + 0.5 * np.eye(n))
    a = (a if np.dtype(dtype).kind == "c" else a.real).astype(dtype)
    truth = ld_cholesky_upper(a)
    same = np.linalg.cholesky(a).conj().transpose(0, 2, 1)
    return _frozen(a, truth, _rel(same, truth))


@pytest.mark.parametrize("dtype", TYPES, ids=_ids)
@pytest.mark.parametrize("n,wave", SIZES)
def test_cholesky_sweep(gpu, n, wave, dtype):
    import torch
    import superbblas_amd as sb
    a, truth, e_lapack = _chol_case(n, dtype)
    dim = list(a.shape)
    v = torch.from_numpy(a.ravel().copy()).to(gpu)
    with _wave(wave):
        sb.cholesky(_full(dim), dim, "tij", [v], "i", "j")
        torch.cuda.synchronize()
    out = v.cpu().numpy().reshape(dim)
    lo = np.tril_indices(n, -1)
    # the strict lower triangle is untouched (potrf_kernel's header comment)
    assert np.array_equal(_bits(out[:, lo[0], lo[1]]), _bits(a[:, lo[0], lo[1]]))
    _check("rand", "cholesky", _path(n, wave), dtype, a, _rel(np.triu(out), truth), e_lapack)
