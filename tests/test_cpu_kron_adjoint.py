"""The reference the GPU tests of the Kronecker adjoint compare against (tests/_kron_adjoint.py:
the dense matrix of A from the oracle's forward product on unit vectors, A^H x with numpy),
checked on its own: <A^H x, z> == <x, A z> exactly for integer x and z, with A z straight from
the oracle's Kronecker product (no dense matrix in between)."""
import numpy as np
import pytest

from _common import T_CDOUBLE, oracle_kron_bsr
from _kron_adjoint import adjoint_ref, forward_ref, int_vector, lattice_case


@pytest.mark.parametrize("bif", [False, True])
@pytest.mark.parametrize("spin,color", [(4, 3), (2, 2)])
@pytest.mark.parametrize("L", [1, 2])
def test_adjoint_reference(L, spin, color, bif):
    V, ncols = L ** 4, 2
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, bif)
    n = V * color * ncols * spin
    x, z = int_vector(n, seed=1), int_vector(n, seed=2)
    az = np.zeros(n, np.complex128)
    oracle_kron_bsr(T_CDOUBLE, [L, L, L, L, 1, 1], 0, V, 9, color, color, spin, spin, jj, vals,
                    kron, bif, z, az, ncols, 1.0)
    assert np.array_equal(az, forward_ref(A, z, V, color, color, spin, spin, ncols))
    ahx = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    assert np.any(ahx != 0)
    # (integers far below 2^53: both sides exact)
    assert np.vdot(ahx, z) == np.vdot(x, az)


def test_adjoint_reference_rectangular():
    """ki != kd and bi != bd: a swapped index in the helper does not cancel out"""
    L, bi, bd, ki, kd, ncols = 2, 3, 2, 2, 4, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, bi, bd, ki, kd, True, False)
    assert A.shape == (V * bi * ki, V * bd * kd)
    x, z = int_vector(V * bi * ncols * ki, seed=3), int_vector(V * bd * ncols * kd, seed=4)
    az = np.zeros(V * bi * ncols * ki, np.complex128)
    oracle_kron_bsr(T_CDOUBLE, [L, L, L, L, 1, 1], 0, V, 9, bi, bd, ki, kd, jj, vals, kron, False,
                    z, az, ncols, 1.0)
    assert np.array_equal(az, forward_ref(A, z, V, bi, bd, ki, kd, ncols))
    assert np.vdot(adjoint_ref(A, x, V, bi, bd, ki, kd, ncols), z) == np.vdot(x, az)
