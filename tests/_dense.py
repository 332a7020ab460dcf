"""Layout helpers for the dense batched solvers (dense.h): the reference's working orders
(prepare_for_cholesky, dense.h:507-560; trsm/gesm 760-770) as numpy transposes, and the golden
inputs of oracle/ref_golden.cpp dense_cases.  Test infrastructure only."""
import numpy as np

from _golden import gen


def _labels(o, orows, ocols):
    ot = [c for c in o if c not in orows and c not in ocols]
    return ot


def to_matrices(v, o, dim, orows, ocols):
    """Tensor (labels o, SlowToFast) -> (nbatch, n, n) with [b, r, c], r / c the row / column
    indices in orows / ocols label order (last label fastest)."""
    ot = _labels(o, orows, ocols)
    order = ot + list(orows) + list(ocols)
    perm = [o.index(c) for c in order]
    a = v.reshape(dim).transpose(perm)
    n = int(np.prod([dim[o.index(c)] for c in orows]))
    return a.reshape(-1, n, n)


def from_matrices(m, o, dim, orows, ocols):
    ot = _labels(o, orows, ocols)
    order = ot + list(orows) + list(ocols)
    perm = [o.index(c) for c in order]
    shp = [dim[i] for i in perm]
    return m.reshape(shp).transpose(np.argsort(perm)).ravel()


def to_panel(v, o, dim, first, second):
    """Tensor -> (nbatch, A, B) with the labels `first` then `second` (batch labels: the rest,
    in o order)."""
    ot = [c for c in o if c not in first and c not in second]
    order = ot + list(first) + list(second)
    perm = [o.index(c) for c in order]
    a = v.reshape(dim).transpose(perm)
    na = int(np.prod([dim[o.index(c)] for c in first]))
    nb = int(np.prod([dim[o.index(c)] for c in second]))
    return a.reshape(-1, na, nb)


def from_panel(m, o, dim, first, second):
    ot = [c for c in o if c not in first and c not in second]
    order = ot + list(first) + list(second)
    perm = [o.index(c) for c in order]
    shp = [dim[i] for i in perm]
    return m.reshape(shp).transpose(np.argsort(perm)).ravel()


def dense_input(kind, nt, n, dtype, seed=3):
    """oracle/ref_golden.cpp dense_input: (nt, n, n) with [t, r, c]."""
    b = gen("int", nt * n * n, seed, dtype).reshape(nt, n, n)
    if kind == "hpd":
        a = np.einsum("tqr,tqc->trc", b.conj(), b) + n * np.eye(n)
    elif kind == "tri":
        a = np.full((nt, n, n), 99, dtype)
        iu = np.triu_indices(n, 1)
        a[:, iu[0], iu[1]] = b[:, iu[0], iu[1]]
        d = np.arange(n)
        a[:, d, d] = n + 3 + np.abs(b[:, d, d])
    else:
        a = b + 4 * n * np.eye(n)
    return a.astype(dtype)


# ---- inputs whose pivots leave the diagonal, and a long-double truth ----

def perm_dominant(nt, n, dtype, seed=11):
    """Row-permuted diagonally dominant matrices: (nt, n, n) [t, r, c] and the permutations
    (row r of matrix t is row perms[t, r] of the dominant matrix).  Small integer entries, so
    the same matrices are exact in all four types; as well conditioned as dense_input("gen"),
    and the pivot sequence of partial pivoting is the one that sorts the permutation
    (implied_pivots).  Matrix 0 carries the n-cycle (every step but the last swaps), matrix 1
    the identity (the unswapped control).  The shift is 4 n + 7: with gen's 4 n the real n = 1
    matrix can be exactly 0."""
    b = gen("int", nt * n * n, seed, dtype).reshape(nt, n, n)
    a = (b + (4 * n + 7) * np.eye(n)).astype(dtype)
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(n) for _ in range(nt)])
    perms[0] = np.roll(np.arange(n), 1)
    if nt > 1:
        perms[1] = np.arange(n)
    return np.take_along_axis(a, perms[:, :, None], axis=1), perms


def implied_pivots(perm):
    """The 0-based pivot rows LAPACK's getrf takes on a perm_dominant matrix: at step j the
    dominant row j, wherever the earlier swaps have left it."""
    cur = list(perm)
    piv = []
    for j in range(len(cur)):
        p = cur.index(j)
        piv.append(p)
        cur[j], cur[p] = cur[p], cur[j]
    return np.array(piv)


def rand_capped(nt, n, dtype, seed=12, cap=1e3):
    """(nt, n, n) matrices of gen("rand") entries in their drawn order, a draw whose 2-norm
    condition number (in complex128) exceeds cap replaced by the next one: the selection looks
    at the input alone."""
    pool = 2 * nt + 8
    a = gen("rand", pool * n * n, seed, dtype).reshape(pool, n, n)
    keep = np.flatnonzero(np.linalg.cond(a.astype(np.complex128)) <= cap)[:nt]
    assert len(keep) == nt, "rand_capped: more than half of the draws exceed the cap"
    return np.ascontiguousarray(a[keep])


def _ld_type(*xs):
    return np.clongdouble if any(np.iscomplexobj(x) for x in xs) else np.longdouble


def ld_solve(a, b):
    """a^-1 b for (nt, n, n) and (nt, n, m): batched Gauss-Jordan elimination with partial
    pivoting on [a | b] in long double (x87: eps ~ 1e-19) -- the high-precision truth, numpy's
    linalg taking no long double."""
    t = _ld_type(a, b)
    w = np.concatenate([a.astype(t), b.astype(t)], axis=2)
    nt, n = a.shape[:2]
    bi = np.arange(nt)
    for j in range(n):
        p = j + np.argmax(np.abs(w[:, j:, j]), axis=1)
        rj, rp = w[bi, j].copy(), w[bi, p].copy()
        w[bi, p] = rj
        w[bi, j] = rp / rp[:, j:j + 1]
        f = w[:, :, j:j + 1].copy()
        f[:, j] = 0
        w -= f * w[:, j:j + 1, :]
    return w[:, :, n:]


def ld_inverse(a):
    return ld_solve(a, np.broadcast_to(np.eye(a.shape[1]), a.shape))


def ld_cholesky_upper(a):
    """U (upper, zero below the diagonal) with a = U^H U, from a's upper triangle and the real
    part of its diagonal alone, in long double."""
    u = a.astype(_ld_type(a))
    for j in range(a.shape[1]):
        d = np.sqrt(u[:, j, j].real)
        u[:, j, j] = d
        u[:, j, j + 1:] /= d[:, None]
        r = u[:, j, j + 1:]
        u[:, j + 1:, j + 1:] -= r.conj()[:, :, None] * r[:, None, :]
    return np.triu(u)
