"""Adjoint of Kronecker BSR operators: bsr_krylov with the image labels on x computes
y = alpha A^H x (+ beta y) for operators made by create_kron_bsr (bsr_kron_adj_kernel, kernel 15,
for 3x3 blocks x 4x4 spin matrices; bsr_kron_adj_generic_kernel, 16, otherwise).  The reference
goes beyond here (its local Kronecker operators throw "unsupported conjugation", bsr.h:399, 1032)
and the oracle has no such product, so the truth is the dense matrix of A from the oracle's forward
product (tests/_kron_adjoint.py, checked on its own by tests/test_cpu_kron_adjoint.py).  Integer
data: |K| <= |3+2i|, |U| <= |3+4i|, |x| <= |3+2i|, 108 terms per output, every partial sum below
7100 << 2^24, so the comparisons are exact in all four types at power 1."""
import numpy as np
import pytest

from _kron_adjoint import (DIRS, adjoint_ref, dense_matrix, int_vector, kron_operator,
                           lattice_case)

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.complex128): "complex128", np.dtype(np.complex64): "complex64",
         np.dtype(np.float64): "float64", np.dtype(np.float32): "float32"}


def make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, dtype=np.complex128):
    import torch
    cplx = np.dtype(dtype).kind == "c"
    cast = (lambda a: a.astype(dtype)) if cplx else (lambda a: a.real.astype(dtype))
    dimi, dimd = [L, L, L, L, ki, bi], [L, L, L, L, kd, bd]
    tv, tk = torch.from_numpy(cast(vals)).to(gpu), torch.from_numpy(cast(kron)).to(gpu)
    op = sb.create_kron_bsr([([0] * 6, dimi)], dimi, [([0] * 6, dimd)], dimd,
                            [1, 1, 1, 1, 1, bi], [1, 1, 1, 1, 1, bd], [1, 1, 1, 1, ki, 1],
                            [1, 1, 1, 1, kd, 1], bif, [torch.from_numpy(np.array(ii)).to(gpu)],
                            [torch.from_numpy(np.array(jj)).to(gpu)], [tv], [tk])
    return op, tv, tk


def apply_adjoint(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, dtype=np.complex128, alpha=1.0,
                  beta=0.0, y0=None, power=1):
    """y (pXYZTCnS) = alpha (A^H)^(p+1) x (pxyztcns) + beta y0; returns (kernel, y as complex128)"""
    import torch
    cplx = np.dtype(dtype).kind == "c"
    cast = (lambda a: a.astype(dtype)) if cplx else (lambda a: a.real.astype(dtype))
    dimx = [1, L, L, L, L, bi, ncols, ki]
    dimy = [power, L, L, L, L, bd, ncols, kd]
    tx = torch.from_numpy(cast(x)).to(gpu)
    ny = int(np.prod(dimy))
    ty = (torch.from_numpy(cast(y0)).to(gpu) if y0 is not None else
          torch.zeros(ny, dtype=getattr(torch, TORCH[np.dtype(dtype)]), device=gpu))
    sb.bsr_krylov(alpha, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pxyztcns", [0] * 8, dimx,
                  dimx, [tx], beta, [([0] * 8, dimy)], "pXYZTCnS", [0] * 8, dimy, dimy, "p", [ty])
    torch.cuda.synchronize()
    return sb.tune_get("bsr.last_kernel"), ty.cpu().numpy().astype(np.complex128)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
@pytest.mark.parametrize("spin,color,ncols", [(4, 3, 3), (2, 3, 2), (4, 1, 5)])
@pytest.mark.parametrize("L", [3, 2, 1])
def test_kron_adjoint_types_sizes(gpu, L, spin, color, ncols, dtype):
    """every type; L = 2: two nonzeros of a row point at the same site, L = 1: all nine;
    (4, 3) runs the specialised kernel, the others the generic one"""
    import superbblas_amd as sb
    real = np.dtype(dtype).kind != "c"
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False, real)
    V = L ** 4
    x = int_vector(V * color * ncols * spin, cplx=not real)
    ref = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, dtype)
    try:
        kernel, out = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x, dtype)
    finally:
        op.destroy()
    assert kernel == (15 if (spin, color) == (4, 3) else 16)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("ncols", [1, 2, 7, 12, 16, 17, 31, 32, 64, 65])
@pytest.mark.parametrize("bif", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_kron_adjoint_kernel_forms(gpu, sparse, bif, ncols, dtype):
    """3x3 x 4x4 on 81 sites: fewer columns than a wave, a wave spanning several sites with a
    ragged tail, a whole wave on one site and one column more (31 and 32 columns: the last count
    whose lanes read their blocks themselves and the first with the blocks staged in LDS; 81
    sites: a last workgroup with fewer sites than the others); sparse and dense spin matrices,
    both block orders, complex alpha, beta 0 and 2; the specialised and the generic kernel
    against the reference and each other"""
    import superbblas_amd as sb
    L, spin, color = 3, 4, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, sparse, bif)
    n = V * color * ncols * spin
    x = int_vector(n)
    y0 = ((np.arange(n) % 7 - 3) + 1j).astype(np.complex128)
    alpha = 1 - 1j
    ahx = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, bif, ii, jj, vals, kron, dtype)
    old = sb.tune_get("bsr.kron_adj")
    outs = {}
    try:
        for on in (1, 0, 2):  # (2: the specialised kernel without its LDS staging)
            sb.tune_set("bsr.kron_adj", on)
            for beta in (0.0, 2.0):
                outs[on, beta] = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x,
                                               dtype, alpha, beta, y0)
    finally:
        sb.tune_set("bsr.kron_adj", old)
        op.destroy()
    for (on, beta), (kernel, out) in outs.items():
        assert kernel == (15 if on else 16), (on, kernel)
        assert np.array_equal(out, alpha * ahx + beta * y0), (on, beta)
    for beta in (0.0, 2.0):
        assert np.array_equal(outs[1, beta][1], outs[0, beta][1])
        assert np.array_equal(outs[1, beta][1], outs[2, beta][1])


def test_kron_adjoint_powers(gpu):
    """the image side with okr: y[p] = alpha (A^H)^(p+1) x, p < 3 (complex<double> only: every
    power multiplies the magnitudes by up to 108 |U| |K|; the test checks that the reference
    stays below 2^50, so every sum is exact)"""
    import superbblas_amd as sb
    L, spin, color, ncols, power = 3, 4, 3, 2, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, True, False)
    n = V * color * ncols * spin
    x = int_vector(n)
    y0 = ((np.arange(n * power) % 5 - 2) - 1j).astype(np.complex128)
    alpha, beta = 1 - 1j, 2.0
    refs, cur = [], x
    for _ in range(power):
        cur = adjoint_ref(A, cur, V, color, color, spin, spin, ncols)
        refs.append(cur)
    assert max(np.abs(r).max() for r in refs) < 2.0 ** 50
    ref = np.concatenate([alpha * r + beta * y0[p * n:(p + 1) * n] for p, r in enumerate(refs)])
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    try:
        _, out = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x, np.complex128,
                               alpha, beta, y0, power)
    finally:
        op.destroy()
    assert np.array_equal(out, ref)


def test_kron_adjoint_just_local_request(gpu):
    """just_local and a deferred request on the image side: one process, so both are the plain
    product (a request is returned only when a halo exchange is left in flight)"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 2, 4, 3, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False)
    x = int_vector(V * color * ncols * spin)
    ref = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    dimx = [1, L, L, L, L, color, ncols, spin]
    outs = []
    try:
        for kw in ({"just_local": True}, {"request": True}):
            ty = torch.zeros(x.size, dtype=torch.complex128, device=gpu)
            req = sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pxyztcns",
                                [0] * 8, dimx, dimx, [torch.from_numpy(x).to(gpu)], 0.0,
                                [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx, dimx, "p", [ty], **kw)
            if req is not None:
                req.wait()
            torch.cuda.synchronize()
            outs.append(ty.cpu().numpy())
    finally:
        op.destroy()
    for out in outs:
        assert np.array_equal(out, ref)


def test_kron_adjoint_other_layouts(gpu):
    """x and y not in the preferred (site, block, C, kron) order: through the temporaries"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False)
    x = int_vector(V * color * ncols * spin)
    ref = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    # preferred: x pxyztcns and y pXYZTCnS; use x = nxyztsc and y = pXYZTSnC instead
    xt = x.reshape(L, L, L, L, color, ncols, spin).transpose(5, 0, 1, 2, 3, 6, 4).copy()
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    dimx = [ncols, L, L, L, L, spin, color]
    dimy = [1, L, L, L, L, spin, ncols, color]
    tx = torch.from_numpy(xt.ravel()).to(gpu)
    ty = torch.zeros(V * color * ncols * spin, dtype=torch.complex128, device=gpu)
    try:
        sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 7, dimx)], "nxyztsc", [0] * 7, dimx,
                      dimx, [tx], 0.0, [([0] * 8, dimy)], "pXYZTSnC", [0] * 8, dimy, dimy, "p",
                      [ty])
        torch.cuda.synchronize()
    finally:
        op.destroy()
    out = ty.cpu().numpy().reshape(L, L, L, L, spin, ncols, color).transpose(0, 1, 2, 3, 6, 5, 4)
    assert np.array_equal(out.ravel(), ref)


@pytest.mark.parametrize("ncols", [2, 20])
def test_kron_adjoint_two_components_halo(gpu, ncols):
    """one process, two components on one device: A's image split in two along x on a 4^4 lattice,
    each component's domain its image plus a one-site halo in every direction (as
    tests/dist_worker.py case_kron builds it per rank).  The halo sites are the rows of A^H with
    fewer entries, and the components' contributions to the same domain site are summed; equal
    to the one-component result and to the reference, bit for bit"""
    import torch
    import superbblas_amd as sb
    L, spin, color = 4, 4, 3
    V = L ** 4
    ii, jj, vals, kron = kron_operator(L, color, color, spin, spin)
    dim = [L, L, L, L, spin, color]
    dom = np.array(dim[:4])
    pi = [([2 * c, 0, 0, 0, 0, 0], [2, L, L, L, spin, color]) for c in range(2)]
    pd = []
    for f, s in pi:
        f, s = list(f), list(s)
        for d in range(4):
            s[d] = min(dim[d], s[d] + 2)
            f[d] = (f[d] - 1) % dim[d] if s[d] < dim[d] else 0
        pd.append((f, s))
    nb = color * color
    allv = vals.reshape(V, 9 * nb)
    cii, cjj, cv, ck = [], [], [], []
    for c in range(2):
        f, s = pi[c]
        sites = np.array(np.unravel_index(np.arange(int(np.prod(s[:4]))), s[:4])).T + np.array(f[:4])
        cj = []
        for st in sites:
            for d, dr in DIRS:
                q = st.copy()
                if d is not None:
                    q[d] += dr
                cj.append(list((q - np.array(pd[c][0][:4])) % dom) + [0, 0])
        gsite = np.ravel_multi_index(tuple((sites % dom).T), dim[:4])
        cii.append(torch.from_numpy(np.full(len(sites), 9, np.int32)).to(gpu))
        cjj.append(torch.from_numpy(np.array(cj, np.int32).ravel()).to(gpu))
        cv.append(torch.from_numpy(np.ascontiguousarray(allv[gsite]).ravel()).to(gpu))
        ck.append(torch.from_numpy(kron.copy()).to(gpu))
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    n = V * color * ncols * spin
    x = int_vector(n)
    # one component: the whole lattice
    op1, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    try:
        kernel1, one = apply_adjoint(sb, gpu, op1, L, color, color, spin, spin, ncols, x)
    finally:
        op1.destroy()
    op2 = sb.create_kron_bsr(pi, dim, pd, dim, blk, blk, kr, kr, False, cii, cjj, cv, ck)
    dimx = [1, L, L, L, L, color, ncols, spin]
    half = [1, 2, L, L, L, color, ncols, spin]
    px = [([0, 2 * c, 0, 0, 0, 0, 0, 0], half) for c in range(2)]
    xs = x.reshape(2, n // 2)
    vx = [torch.from_numpy(xs[c].copy()).to(gpu) for c in range(2)]
    vy = [torch.full((n // 2,), 7.0, dtype=torch.complex128, device=gpu) for c in range(2)]
    try:
        sb.bsr_krylov(1.0, op2, "xyztsc", "XYZTSC", px, "pxyztcns", [0] * 8, dimx, dimx, vx, 0.0,
                      px, "pXYZTCnS", [0] * 8, dimx, dimx, "p", vy)
        torch.cuda.synchronize()
        kernel2 = sb.tune_get("bsr.last_kernel")
    finally:
        op2.destroy()
    two = np.concatenate([v.cpu().numpy() for v in vy])
    assert kernel1 == 15 and kernel2 == 15
    assert np.array_equal(two, one)
    A = lattice_case(L, color, color, spin, spin, False, False)[4]
    assert np.array_equal(one, adjoint_ref(A, x, V, color, color, spin, spin, ncols))


@pytest.mark.parametrize("ncols", [2, 40])
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_kron_adjoint_hot_and_empty_sites(gpu, dtype, ncols):
    """all 729 nonzeros of an 81-site operator point at sites 0, 1 and 2: rows of A^H with
    hundreds of entries (at 40 columns more than one staging pass of the specialised kernel
    holds, a site's entries spanning passes) and 78 sites nothing points at, whose y is still written (zero;
    beta y under beta); both kernels"""
    import superbblas_amd as sb
    L, spin, color = 3, 4, 3
    V = L ** 4
    ii, _, vals, kron = kron_operator(L, color, color, spin, spin, True)
    I, mu = np.divmod(np.arange(V * 9), 9)
    jj = np.zeros((V * 9, 6), np.int32)
    jj[:, 3] = (I * 2 + mu * mu) % 3  # (the t coordinate: sites 0, 1, 2)
    jj = jj.ravel()
    A = dense_matrix(L, color, color, spin, spin, jj, vals, kron, False)
    n = V * color * ncols * spin
    x = int_vector(n)
    y0 = ((np.arange(n) % 5 - 2) + 2j).astype(np.complex128)
    ahx = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    assert np.abs(ahx).max() < 2 ** 23 and not np.any(ahx.reshape(V, -1)[3:])
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, dtype)
    old = sb.tune_get("bsr.kron_adj")
    outs = {}
    try:
        for on in (1, 0):
            sb.tune_set("bsr.kron_adj", on)
            for beta in (0.0, 2.0):
                outs[on, beta] = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x,
                                               dtype, 1.0, beta, y0)
    finally:
        sb.tune_set("bsr.kron_adj", old)
        op.destroy()
    for (on, beta), (kernel, out) in outs.items():
        assert kernel == (15 if on else 16), (on, kernel)
        assert np.array_equal(out, ahx + beta * y0), (on, beta)


@pytest.mark.parametrize("bif", [False, True])
@pytest.mark.parametrize("dtype", [np.complex128, np.float32])
def test_kron_adjoint_rectangular(gpu, dtype, bif):
    """ki != kd and bi != bd (Kronecker matrices 2 x 4, blocks 3 x 2) on the generic kernel: a
    swapped index does not cancel out"""
    import superbblas_amd as sb
    L, bi, bd, ki, kd, ncols = 2, 3, 2, 2, 4, 3
    V = L ** 4
    real = np.dtype(dtype).kind != "c"
    ii, jj, vals, kron, A = lattice_case(L, bi, bd, ki, kd, True, bif, real)
    x = int_vector(V * bi * ncols * ki, cplx=not real)
    ref = adjoint_ref(A, x, V, bi, bd, ki, kd, ncols)
    op, _, _ = make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, dtype)
    try:
        kernel, out = apply_adjoint(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, dtype)
    finally:
        op.destroy()
    assert kernel == 16
    assert out.size == V * bd * ncols * kd and np.array_equal(out, ref)


@pytest.mark.parametrize("on", [1, 0])
def test_kron_adjoint_matches_forward_random(gpu, on):
    """random complex<double> values, both products from the library:
    |<A^H x, z> - <x, A z>| <= 1e-12 |x| |A|_F |z| (at L = 3 the nine nonzeros of a row point at
    nine sites, so |A|_F^2 = sum_k |U_k|_F^2 |K_mu|_F^2)"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 5
    V = L ** 4
    rng = np.random.default_rng(17)
    ii, jj, _, _ = kron_operator(L, color, color, spin, spin)
    vals = rng.standard_normal(V * 81) + 1j * rng.standard_normal(V * 81)
    kron = rng.standard_normal(144) + 1j * rng.standard_normal(144)
    n = V * color * ncols * spin
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    normA = np.sqrt(((np.abs(vals.reshape(V, 9, 9)) ** 2).sum(axis=(0, 2)) *
                     (np.abs(kron.reshape(9, 16)) ** 2).sum(axis=1)).sum())
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    dimx = [1, L, L, L, L, color, ncols, spin]
    old = sb.tune_get("bsr.kron_adj")
    try:
        sb.tune_set("bsr.kron_adj", on)
        _, ahx = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x)
        taz = torch.zeros(n, dtype=torch.complex128, device=gpu)
        sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx,
                      dimx, [torch.from_numpy(z).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztcns",
                      [0] * 8, dimx, dimx, "p", [taz])
        torch.cuda.synchronize()
    finally:
        sb.tune_set("bsr.kron_adj", old)
        op.destroy()
    az = taz.cpu().numpy()
    diff = abs(np.vdot(ahx, z) - np.vdot(x, az))
    bound = 1e-12 * np.linalg.norm(x) * normA * np.linalg.norm(z)
    print("adjoint consistency: diff %.3e bound %.3e" % (diff, bound))
    assert np.abs(ahx).max() > 0 and diff <= bound


def test_kron_adjoint_values_in_place(gpu):
    """A^H reads the caller's values and spin matrices in place: after they are overwritten on the
    device the same handle applies the adjoint of the new operator"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 2, 4, 3, 4
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False)
    x = int_vector(V * color * ncols * spin)
    vals2 = np.conj(vals[::-1]) + 1
    kron2 = np.conj(kron[::-1]) - 1j
    A2 = dense_matrix(L, color, color, spin, spin, jj, vals2, kron2, False)
    op, tv, tk = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    try:
        _, out1 = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x)
        tv.copy_(torch.from_numpy(vals2.copy()))
        tk.copy_(torch.from_numpy(kron2.copy()))
        _, out2 = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x)
    finally:
        op.destroy()
    assert np.array_equal(out1, adjoint_ref(A, x, V, color, color, spin, spin, ncols))
    ref2 = adjoint_ref(A2, x, V, color, color, spin, spin, ncols)
    assert not np.array_equal(out1, ref2) and np.array_equal(out2, ref2)


@pytest.mark.parametrize("seed", range(16))
def test_kron_adjoint_fuzz(gpu, seed):
    """random Kronecker operators: lattice 1-3, spin 1 / 2 / 4, color 1-3, rhs columns 1-300
    (log-uniform), every type, either block order, sparse or dense spin matrices.  Exact."""
    import superbblas_amd as sb
    rng = np.random.default_rng(4200 + seed)
    dtype = [np.complex128, np.complex64, np.float64, np.float32][seed % 4]
    real = np.dtype(dtype).kind != "c"
    L = int(rng.integers(1, 4))
    spin = int(rng.choice([1, 2, 4]))
    color = int(rng.choice([1, 2, 3, 3]))
    if seed % 3 == 0:
        spin, color = 4, 3  # the specialised kernel
    ncols = int(np.exp(rng.uniform(0, np.log(300))))
    bif = bool(rng.integers(0, 2))
    sparse = bool(rng.integers(0, 2))
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, sparse, bif, real)
    x = int_vector(V * color * ncols * spin, cplx=not real, seed=seed)
    ref = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, bif, ii, jj, vals, kron, dtype)
    try:
        kernel, out = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x, dtype)
    finally:
        op.destroy()
    assert kernel == (15 if (spin, color) == (4, 3) else 16)
    assert np.array_equal(out, ref), (dtype, L, spin, color, ncols, bif, sparse, kernel)
