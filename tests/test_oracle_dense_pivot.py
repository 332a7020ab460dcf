"""The inputs and the truth of tests/test_gpu_dense_pivot.py, pinned on the CPU: the long-double
elimination of tests/_dense.py against numpy's LAPACK, and the oracle's getrf / getrs (its
pivoting as untested as the GPU's before) against it on matrices whose pivots leave the
diagonal, with the pivot rows the permutation implies."""
import numpy as np
import pytest

from _common import oracle_getrf, oracle_getrs
from _dense import implied_pivots, ld_inverse, perm_dominant, rand_capped

TYPES = [np.complex128, np.float64, np.complex64, np.float32]
SIZES = [1, 2, 4, 7, 12, 16, 17, 33]
NT = 6
EPS64 = np.finfo(np.float64).eps


def _dense_tol(t):
    """as tests/test_oracle_golden.py: relative to the largest entry"""
    return 1e-12 if np.dtype(t) in (np.float64, np.complex128) else 1e-5


def _family(kind, n, dtype):
    return perm_dominant(NT, n, dtype)[0] if kind == "perm" else rand_capped(NT, n, dtype)


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["perm", "rand"])
def test_ld_inverse_matches_lapack(kind, n, dtype):
    a = _family(kind, n, dtype)
    assert a.dtype == dtype and a.shape == (NT, n, n)
    truth = ld_inverse(a)
    ref = np.linalg.inv(a.astype(np.complex128))
    cond = np.linalg.cond(a.astype(np.complex128))
    if kind == "rand":
        assert cond.max() <= 1e3
    err = np.abs(truth - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    assert (err <= 16 * n * EPS64 * cond).all(), (err, cond)
    # and it is an inverse to long-double accuracy
    res = np.abs(np.einsum("trk,tkc->trc", a.astype(truth.dtype), truth) - np.eye(n)).max()
    assert res < 1e-15 * n * cond.max()


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_lu_pivots(n, dtype):
    a, perms = perm_dominant(NT, n, dtype)
    w = np.ascontiguousarray(a.transpose(0, 2, 1)).ravel()  # column-major per matrix
    piv = np.zeros(NT * n, np.int32)
    assert oracle_getrf(w, n, NT, piv) == 0
    piv = piv.reshape(NT, n)
    # oracle.c stores LAPACK's 1-based rows
    for t in range(NT):
        assert np.array_equal(piv[t] - 1, implied_pivots(perms[t])), t
    assert np.count_nonzero(piv[0] - 1 != np.arange(n)) == n - 1  # the n-cycle: every step but the last
    assert np.array_equal(piv[1] - 1, np.arange(n))                # the control: none
    eye = np.tile(np.eye(n, dtype=dtype).ravel(), NT)
    assert oracle_getrs(w, n, NT, piv.ravel(), n, eye) == 0
    res = eye.reshape(NT, n, n).transpose(0, 2, 1)
    truth = ld_inverse(a)
    assert np.abs(res - truth).max() <= _dense_tol(dtype) * np.abs(truth).max()


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_rand_capped_selection(n, dtype):
    """the draws kept are a subsequence of the generator's, the same in every call"""
    a = rand_capped(NT, n, dtype)
    assert np.array_equal(a, rand_capped(NT, n, dtype))
    assert np.array_equal(a[:3], rand_capped(3, n, dtype))
    assert np.linalg.cond(a.astype(np.complex128)).max() <= 1e3
