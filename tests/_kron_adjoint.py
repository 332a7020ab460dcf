"""Reference for the adjoint of a Kronecker BSR operator (x with the image labels): the oracle
has no adjoint Kronecker product, so the dense matrix of A is built from the oracle's forward
product (oracle_kron_bsr) applied to the unit vectors, and A^H x is taken with numpy.  Integer
data as in tests/test_gpu_kron_bsr.py (kron_lattice): |K| <= |3+2i|, |U| <= |3+4i|, exact in every
type at power 1."""
import functools

import numpy as np

from _common import T_CDOUBLE, oracle_kron_bsr

DIRS = [(None, 0)] + [(d, dr) for d in range(4) for dr in (-1, 1)]


def kron_operator(L, bi, bd, ki, kd, sparse_kron=False):
    """The 9-point stencil on an L^4 periodic lattice: bi x bd blocks, ki x kd Kronecker matrices
    (for bi == bd and ki == kd the data of test_gpu_kron_bsr.kron_lattice)."""
    V = L ** 4
    sites = np.array(np.unravel_index(np.arange(V), (L, L, L, L))).T
    jj = []
    for s in sites:
        for d, dr in DIRS:
            c = s.copy()
            if d is not None:
                c[d] = (c[d] + dr) % L
            jj.append(list(c) + [0, 0])
    jj = np.array(jj, np.int32).ravel()
    k = np.arange(V * 9 * bi * bd, dtype=np.int64)
    vals = ((k * 3 + 1) % 7 - 3) + 1j * ((k * 5 + 2) % 9 - 4)
    q = np.arange(9 * ki * kd, dtype=np.int64)
    kron = ((q * 5 + 2) % 7 - 3) + 1j * ((q * 3 + 1) % 5 - 2)
    if sparse_kron:
        # Wilson-projector-like pattern: half of every matrix is zero (the skip path)
        a, b = np.unravel_index(q % (ki * kd), (ki, kd))
        kron[(a + b + q // (ki * kd)) % 2 == 1] = 0
    return np.full(V, 9, np.int32), jj, vals.astype(np.complex128), kron.astype(np.complex128)


def dense_matrix(L, bi, bd, ki, kd, jj, vals, kron, bif):
    """A as a dense (V bi ki) x (V bd kd) matrix, rows (I, i, a) and columns (J, d, b): one
    forward product of the oracle with the identity as x (one rhs column per unit vector)."""
    V = L ** 4
    nd, ni = V * bd * kd, V * bi * ki
    # x (site, d, col, b) = 1 where col is the index of (site, d, b)
    x = np.zeros((V * bd, nd, kd), np.complex128)
    col = np.arange(nd).reshape(V * bd, kd)
    for b in range(kd):
        x[np.arange(V * bd), col[:, b], b] = 1
    y = np.zeros(ni * nd, np.complex128)
    oracle_kron_bsr(T_CDOUBLE, [L, L, L, L, 1, 1], 0, V, 9, bi, bd, ki, kd, jj,
                    np.ascontiguousarray(vals, np.complex128),
                    np.ascontiguousarray(kron, np.complex128), bif, x.ravel(), y, nd, 1.0)
    return y.reshape(V * bi, nd, ki).transpose(0, 2, 1).reshape(ni, nd)


@functools.lru_cache(maxsize=None)
def lattice_case(L, bi, bd, ki, kd, sparse=False, bif=False, real=False):
    """(ii, jj, vals, kron, A) of kron_operator, computed once per case and shared (read only)"""
    ii, jj, vals, kron = kron_operator(L, bi, bd, ki, kd, sparse)
    if real:
        vals, kron = vals.real.astype(np.complex128), kron.real.astype(np.complex128)
    A = dense_matrix(L, bi, bd, ki, kd, jj, vals, kron, bif)
    for a in (ii, jj, vals, kron, A):
        a.setflags(write=False)
    return ii, jj, vals, kron, A


def forward_ref(A, z, V, bi, bd, ki, kd, ncols):
    """A z for z in the layout (site, d, col, b); the result in (site, i, col, a)"""
    Z = z.reshape(V * bd, ncols, kd).transpose(0, 2, 1).reshape(V * bd * kd, ncols)
    return (A @ Z).reshape(V * bi, ki, ncols).transpose(0, 2, 1).ravel()


def adjoint_ref(A, x, V, bi, bd, ki, kd, ncols):
    """A^H x for x in the layout (site, i, col, a); the result in (site, d, col, b)"""
    X = x.reshape(V * bi, ncols, ki).transpose(0, 2, 1).reshape(V * bi * ki, ncols)
    return (A.conj().T @ X).reshape(V * bd, kd, ncols).transpose(0, 2, 1).ravel()


def int_vector(n, cplx=True, seed=0):
    g = np.arange(n, dtype=np.int64) + 13 * seed
    return ((g % 7 - 3) + (1j * (g % 5 - 2) if cplx else 0)).astype(np.complex128)
