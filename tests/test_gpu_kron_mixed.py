"""Mixed-precision Kronecker operators ("bsr.kron_mixed" 1): an operator of create_kron_bsr in
float / complex<float> (colour blocks and spin matrices) applied by bsr_krylov to double /
complex<double> vectors, A x and A^H x.  The values are read in place and widened exactly, so the
result is the product of the up-converted operator with x: the references are the oracle's
forward product in the double type on vals.astype(double type) (test_gpu_kron_bsr.reference) and,
for A^H, the dense matrix of _kron_adjoint.  Integer data of kron_lattice / lattice_case:
|U| <= 5, |K| <= 4, |x| <= 8 and 9 * 3 * 4 terms per output, so every sum is an integer far below
2^24 in any order (a second power stays below 2^53) and the comparisons are exact.  With the key
at 0 the pair stays refused (tests/test_gpu_bsr_mixed.py::test_mixed_refused_kronecker)."""
import functools

import numpy as np
import pytest

from _common import T_CDOUBLE, oracle_kron_bsr
from _kron_adjoint import adjoint_ref, dense_matrix, int_vector, lattice_case
from test_gpu_kron_bsr import kron_lattice, reference

pytestmark = pytest.mark.gpu

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
WIDE = {C64: C128, F32: F64}
ALPHA, BETA = 1 - 1j, 2.0


@pytest.fixture(autouse=True)
def kron_mixed_on(gpu):
    """the key at 1 for the test, put back afterwards"""
    import superbblas_amd as sb
    old = sb.tune_get("bsr.kron_mixed")
    sb.tune_set("bsr.kron_mixed", 1)
    yield
    sb.tune_set("bsr.kron_mixed", old)


def cast(a, dtype):
    return np.ascontiguousarray(a.astype(dtype) if np.dtype(dtype).kind == "c" else a.real.astype(dtype))


def device_tensor(a, gpu, lead=0):
    """a host array on the device; lead: the tensor starts that many elements into its buffer,
    which ends with the array's last element"""
    import torch
    buf = torch.empty(a.size + lead, dtype=torch.from_numpy(a[:1]).dtype, device=gpu)
    t = buf[lead:]
    t.copy_(torch.from_numpy(a))
    return t


def make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, vt, lead=0):
    """(operator, value tensor, spin-matrix tensor), values and spin matrices in vt"""
    import torch
    dimi, dimd = [L, L, L, L, ki, bi], [L, L, L, L, kd, bd]
    tv, tk = device_tensor(cast(vals, vt), gpu, lead), device_tensor(cast(kron, vt), gpu)
    op = sb.create_kron_bsr([([0] * 6, dimi)], dimi, [([0] * 6, dimd)], dimd,
                            [1, 1, 1, 1, 1, bi], [1, 1, 1, 1, 1, bd], [1, 1, 1, 1, ki, 1],
                            [1, 1, 1, 1, kd, 1], bif, [torch.from_numpy(np.array(ii)).to(gpu)],
                            [torch.from_numpy(np.array(jj)).to(gpu)], [tv], [tk])
    return op, tv, tk


def apply(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, xt, alpha=1.0, beta=0.0, y0=None, power=1,
          adjoint=False, **kw):
    """forward: y (pxyztcns) = alpha A^(p+1) x (pXYZTCnS) + beta y0; adjoint: the labels swapped.
    Returns (last_kernel, last_mixed, y as complex128)"""
    import torch
    if adjoint:
        dimx, dimy = [1, L, L, L, L, bi, ncols, ki], [power, L, L, L, L, bd, ncols, kd]
        ox, oy = "pxyztcns", "pXYZTCnS"
    else:
        dimx, dimy = [1, L, L, L, L, bd, ncols, kd], [power, L, L, L, L, bi, ncols, ki]
        ox, oy = "pXYZTCnS", "pxyztcns"
    tx = torch.from_numpy(cast(x, xt)).to(gpu)
    ty = torch.from_numpy(cast(y0 if y0 is not None else np.zeros(int(np.prod(dimy)), C128), xt)).to(gpu)
    req = sb.bsr_krylov(alpha, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                        [tx], beta, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy, "p", [ty], **kw)
    if req is not None:
        req.wait()
    torch.cuda.synchronize()
    return sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed"), ty.cpu().numpy().astype(C128)


def forward_x(n, power):
    g = np.arange(n)
    x = ((g % 5 - 2) + 1j * (g % 3 - 1)).astype(C128)
    y0 = ((np.arange(n * power) % 7 - 3) + 1j).astype(C128)
    return x, y0


@functools.lru_cache(maxsize=None)
def forward_case(L, spin, color, ncols, bif, sparse, power, real=False):
    """(ii, jj, vals, kron, x, y0, reference) of the 9-point lattice, computed once and shared"""
    ii, jj, vals, kron = kron_lattice(L, spin, color, sparse_kron=sparse)
    x, y0 = forward_x(L ** 4 * color * ncols * spin, power)
    if real:
        vals, kron, x, y0 = (a.real.astype(C128) for a in (vals, kron, x, y0))
    alpha = 2.0 if real else ALPHA
    # (the values through the operator's type and back: exact on this data, asserted)
    vt = F32 if real else C64
    assert np.array_equal(cast(vals, vt).astype(C128), vals) and np.array_equal(cast(kron, vt).astype(C128), kron)
    ref = reference(L, spin, color, ncols, vals.astype(C128), kron.astype(C128), jj, x, alpha, BETA, y0,
                    power, bif)
    for a in (ii, jj, vals, kron, x, y0, ref):
        a.setflags(write=False)
    return ii, jj, vals, kron, x, y0, ref


# (ncols, L): bsr_kron_kernel, the LDS VALU form, packed slots, one row per wave; L = 3: 81 sites,
# a last workgroup with fewer rows than its slots; 40 columns at L = 3: runs starting at an odd
# value index (the 16-byte alignment case of an LDS-DMA staging)
FORWARD = [(1, 4, 0), (3, 4, 0), (4, 4, 0), (7, 4, 0), (8, 4, 6), (12, 4, 6), (12, 3, 6), (8, 3, 6),
           (16, 4, 5), (17, 4, 5), (40, 4, 5), (16, 3, 5), (17, 3, 5), (40, 3, 5)]


@pytest.mark.parametrize("ncols,L,form", FORWARD)
@pytest.mark.parametrize("bif,sparse", [(False, False), (True, True)])
def test_kron_mixed_forward_forms(gpu, ncols, L, form, bif, sparse):
    """complex<float> values under complex<double> vectors, 3x3 (x) 4x4, complex alpha, beta 2,
    power 2: every forward form and every variant of the matrix-core forms (x staged 1-3
    neighbours ahead or loaded per lane, y per lane or through the ring, packing off, MFMA off)
    gives the reference, bit for bit"""
    import superbblas_amd as sb
    spin, color, power = 4, 3, 2
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, bif, sparse, power)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, bif, ii, jj, vals, kron, C64)
    keys = ("bsr.kron_mfma", "bsr.kron_pack", "bsr.kron_xlds", "bsr.kron_ylds", "bsr.kron_spin")
    old = [sb.tune_get(k) for k in keys]
    outs = []
    variants = [(1, 1, 1, 0), (1, 1, 2, 1), (1, 1, 3, 0), (1, 1, 0, 0), (1, 0, 2, 1), (1, 0, 3, 0),
                (1, 0, 0, 0), (0, 1, 1, 1)] if form else [(1, 1, 2, 1), (0, 1, 2, 0)]
    try:
        for on, pack, xl, yl in variants:
            for k, v in zip(keys, (on, pack, xl, yl, 0)):
                sb.tune_set(k, v)
            outs.append(apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA, BETA, y0,
                              power))
    finally:
        for k, v in zip(keys, old):
            sb.tune_set(k, v)
        op.destroy()
    if form:
        assert [o[0] for o in outs] == [form] * 4 + [5] * 3 + [0], [o[0] for o in outs]
    else:
        assert [o[0] for o in outs] == [0, 0]
    for kernel, mixed, out in outs:
        assert mixed == 1
        assert np.array_equal(out, ref), kernel


@pytest.mark.parametrize("ncols", [1, 2, 3, 4, 5, 6, 7])
def test_kron_mixed_low_columns(gpu, ncols):
    """the matrix-core forms below 8 columns ("bsr.kron_mfma_min_cols" 1), 3^4 sites: the packed
    kernel with 2-4 waves and 32, 32, 16, 16 and 8 rows per workgroup at 1, 2, 3, 4 and 6 columns,
    the one-row-per-wave kernel at 5 and 7 and with packing off; a short last workgroup in each"""
    import superbblas_amd as sb
    L, spin, color, power = 3, 4, 3, 2
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, False, False, power)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    keys = ("bsr.kron_mfma_min_cols", "bsr.kron_pack", "bsr.kron_xlds", "bsr.kron_ylds", "bsr.kron_spin",
            "bsr.kron_mfma")
    old = [sb.tune_get(k) for k in keys]
    variants = ((1, 1, 0), (1, 3, 1), (1, 0, 0), (0, 2, 1))
    outs = []
    try:
        for pack, xl, yl in variants:
            for k, v in zip(keys, (1, pack, xl, yl, 0, 1)):
                sb.tune_set(k, v)
            outs.append(apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA, BETA, y0,
                              power))
    finally:
        for k, v in zip(keys, old):
            sb.tune_set(k, v)
        op.destroy()
    for (pack, xl, yl), (kernel, mixed, out) in zip(variants, outs):
        assert kernel == (6 if pack and ncols in (1, 2, 3, 4, 6) else 5), (pack, xl, yl, kernel)
        assert mixed == 1
        assert np.array_equal(out, ref), (pack, xl, yl, kernel)


def test_kron_mixed_spin_first_not_taken(gpu):
    """bsr.kron_spin 1 / 2 (the spin-first kernels read tables of doubles): a mixed launch keeps
    the matrix-core form and the result"""
    import superbblas_amd as sb
    L, spin, color, ncols, power = 3, 4, 3, 12, 2
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, True, True, power)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, True, ii, jj, vals, kron, C64)
    old = sb.tune_get("bsr.kron_spin")
    outs = []
    try:
        for on in (1, 2):
            sb.tune_set("bsr.kron_spin", on)
            outs.append(apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA, BETA, y0, power))
    finally:
        sb.tune_set("bsr.kron_spin", old)
        op.destroy()
    for kernel, mixed, out in outs:
        assert (kernel, mixed) == (6, 1) and np.array_equal(out, ref)


@pytest.mark.parametrize("ncols", [12, 40])
def test_kron_mixed_unaligned_values(gpu, ncols):
    """the value tensor starts one element into its buffer (8 bytes off a 16-byte boundary) and
    ends with the operator's last value: nothing may be read past it, whatever the staging"""
    import superbblas_amd as sb
    L, spin, color, power = 3, 4, 3, 2
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, False, False, power)
    op, tv, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64, lead=1)
    assert tv.data_ptr() % 16 == 8 and tv.numel() == L ** 4 * 81
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA, BETA,
                                   y0, power)
    finally:
        op.destroy()
    assert (kernel, mixed) == (6 if ncols == 12 else 5, 1)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("vt,spin,color,ncols", [(F32, 4, 3, 3), (F32, 4, 3, 12), (F32, 2, 3, 2), (F32, 4, 1, 5),
                                                 (C64, 2, 3, 2), (C64, 4, 1, 5)])
def test_kron_mixed_valu_and_generic(gpu, vt, spin, color, ncols):
    """float -> double on the VALU forms ((4, 3): bsr_kron_kernel at 3 columns, the LDS form at
    12) and both pairs on the generic kernel ((2, 3) and (4, 1))"""
    import superbblas_amd as sb
    L, real = 4, vt == F32
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, False, False, 1, real)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, vt)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, WIDE[vt],
                                   2.0 if real else ALPHA, BETA, y0)
    finally:
        op.destroy()
    assert (kernel, mixed) == (0, 1)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("vt", [C64, F32])
@pytest.mark.parametrize("ncols,L", [(1, 3), (7, 3), (12, 3), (32, 3), (65, 3), (12, 2)])
@pytest.mark.parametrize("bif,sparse", [(False, False), (True, True)])
def test_kron_mixed_adjoint_forms(gpu, bif, sparse, ncols, L, vt):
    """A^H, both pairs, 3x3 (x) 4x4: a lane reading its blocks itself (below 32 columns) and the
    blocks staged in LDS (32, 65), form 15; the generic adjoint kernel (bsr.kron_adj 0), 19 when
    mixed; complex alpha, beta 0 and 2; L = 2: two nonzeros of a row point at one site"""
    import superbblas_amd as sb
    spin, color, real = 4, 3, vt == F32
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, sparse, bif, real)
    n = V * color * ncols * spin
    x = int_vector(n, cplx=not real)
    y0 = ((np.arange(n) % 7 - 3) + (0 if real else 1j)).astype(C128)
    alpha = 2.0 if real else ALPHA
    ahx = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, bif, ii, jj, vals, kron, vt)
    old = sb.tune_get("bsr.kron_adj")
    outs = {}
    try:
        for on in (1, 0):
            sb.tune_set("bsr.kron_adj", on)
            for beta in (0.0, 2.0):
                outs[on, beta] = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, WIDE[vt], alpha,
                                       beta, y0, adjoint=True)
    finally:
        sb.tune_set("bsr.kron_adj", old)
        op.destroy()
    for (on, beta), (kernel, mixed, out) in outs.items():
        assert (kernel, mixed) == (15 if on else 19, 1), (on, kernel, mixed)
        assert np.array_equal(out, alpha * ahx + beta * y0), (on, beta)


@pytest.mark.parametrize("vt", [C64, F32])
def test_kron_mixed_adjoint_generic_sizes(gpu, vt):
    """(spin, colour) = (2, 3): the generic adjoint kernel whatever bsr.kron_adj, 19 when mixed"""
    import superbblas_amd as sb
    L, spin, color, ncols, real = 3, 2, 3, 2, vt == F32
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False, real)
    x = int_vector(V * color * ncols * spin, cplx=not real)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, vt)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, WIDE[vt],
                                   adjoint=True)
    finally:
        op.destroy()
    assert (kernel, mixed) == (19, 1)
    assert np.array_equal(out, adjoint_ref(A, x, V, color, color, spin, spin, ncols))


@pytest.mark.parametrize("bif", [False, True])
@pytest.mark.parametrize("vt", [C64, F32])
def test_kron_mixed_rectangular(gpu, vt, bif):
    """ki != kd and bi != bd (Kronecker matrices 2 x 4, blocks 3 x 2): A x and A^H x on the
    generic kernels, a swapped index does not cancel out"""
    import superbblas_amd as sb
    from _kron_adjoint import forward_ref
    L, bi, bd, ki, kd, ncols, real = 2, 3, 2, 2, 4, 3, vt == F32
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, bi, bd, ki, kd, True, bif, real)
    x = int_vector(V * bi * ncols * ki, cplx=not real)
    z = int_vector(V * bd * ncols * kd, cplx=not real, seed=3)
    op, _, _ = make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, vt)
    try:
        ka, ma, adj = apply(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, WIDE[vt], adjoint=True)
        kf, mf, fwd = apply(sb, gpu, op, L, bi, bd, ki, kd, ncols, z, WIDE[vt])
    finally:
        op.destroy()
    assert (ka, ma, kf, mf) == (19, 1, 0, 1)
    assert adj.size == V * bd * ncols * kd and np.array_equal(adj, adjoint_ref(A, x, V, bi, bd, ki, kd, ncols))
    assert fwd.size == V * bi * ncols * ki and np.array_equal(fwd, forward_ref(A, z, V, bi, bd, ki, kd, ncols))


@pytest.mark.parametrize("ncols", [3, 12, 40])
def test_kron_mixed_values_in_place(gpu, ncols):
    """no snapshot and no converted copy: after the caller overwrites the values and the spin
    matrices on the device, A x and A^H x of the same handle are those of the new operator"""
    import torch
    import superbblas_amd as sb
    from _kron_adjoint import forward_ref
    L, spin, color = 2, 4, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False)
    x = int_vector(V * color * ncols * spin)
    vals2 = np.conj(vals[::-1]) + 1
    kron2 = np.conj(kron[::-1]) - 1j
    A2 = dense_matrix(L, color, color, spin, spin, jj, vals2, kron2, False)
    op, tv, tk = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    args = (sb, gpu, op, L, color, color, spin, spin, ncols, x, C128)
    try:
        f1, a1 = apply(*args)[2], apply(*args, adjoint=True)[2]
        tv.copy_(torch.from_numpy(cast(vals2, C64)))
        tk.copy_(torch.from_numpy(cast(kron2, C64)))
        f2, a2 = apply(*args)[2], apply(*args, adjoint=True)[2]
    finally:
        op.destroy()
    dims = (V, color, color, spin, spin, ncols)
    assert np.array_equal(f1, forward_ref(A, x, *dims)) and np.array_equal(a1, adjoint_ref(A, x, *dims))
    rf, ra = forward_ref(A2, x, *dims), adjoint_ref(A2, x, *dims)
    assert not np.array_equal(f1, rf) and not np.array_equal(a1, ra)
    assert np.array_equal(f2, rf) and np.array_equal(a2, ra)


def test_kron_mixed_other_layouts(gpu):
    """x and y in layouts other than the preferred (D, d, C, kd): through the temporaries, which
    take x's type"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 4, 4, 3, 3
    ii, jj, vals, kron, x, _, _ = forward_case(L, spin, color, ncols, False, False, 1)
    V = L ** 4
    ref = reference(L, spin, color, ncols, vals, kron, jj, x, 1.0, 0.0, np.zeros_like(x), 1)
    # preferred: x pXYZTCnS and y pxyztcns; use x = nXYZTSC (column major) and y = pxyztsnc
    xt = x.reshape(L, L, L, L, color, ncols, spin).transpose(5, 0, 1, 2, 3, 6, 4).copy()
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    dimx = [ncols, L, L, L, L, spin, color]
    dimy = [1, L, L, L, L, spin, ncols, color]
    tx = torch.from_numpy(xt.ravel()).to(gpu)
    ty = torch.zeros(V * color * ncols * spin, dtype=torch.complex128, device=gpu)
    try:
        sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 7, dimx)], "nXYZTSC", [0] * 7, dimx,
                      dimx, [tx], 0.0, [([0] * 8, dimy)], "pxyztsnc", [0] * 8, dimy, dimy, "p", [ty])
        torch.cuda.synchronize()
        mixed = sb.tune_get("bsr.last_mixed")
    finally:
        op.destroy()
    out = ty.cpu().numpy().reshape(L, L, L, L, spin, ncols, color).transpose(0, 1, 2, 3, 6, 5, 4)
    assert mixed == 1 and np.array_equal(out.ravel(), ref)


@pytest.mark.parametrize("adjoint", [False, True])
def test_kron_mixed_just_local_request(gpu, adjoint):
    """just_local and a deferred request: one process, so both are the plain product"""
    import superbblas_amd as sb
    from _kron_adjoint import forward_ref
    L, spin, color, ncols = 2, 4, 3, 3
    V = L ** 4
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin, False, False)
    x = int_vector(V * color * ncols * spin)
    ref = (adjoint_ref if adjoint else forward_ref)(A, x, V, color, color, spin, spin, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    try:
        outs = [apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, adjoint=adjoint, **kw)
                for kw in ({"just_local": True}, {"request": True})]
    finally:
        op.destroy()
    for _, mixed, out in outs:
        assert mixed == 1 and np.array_equal(out, ref)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("ncols", [2, 20])
def test_kron_mixed_two_components_halo(gpu, ncols, adjoint):
    """one process, two components on one device: A's image split in two along x on a 4^4 lattice,
    each component's domain its image plus a one-site halo in every direction (as
    test_gpu_kron_adjoint.test_kron_adjoint_two_components_halo builds it); x reaches the domain
    partition through the halo exchange in complex<double>, and for A^H the components'
    contributions to one domain site are summed"""
    import torch
    import superbblas_amd as sb
    from _kron_adjoint import DIRS, forward_ref, kron_operator
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
    allv = vals.reshape(V, 9 * color * color)
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
        cv.append(torch.from_numpy(cast(np.ascontiguousarray(allv[gsite]).ravel(), C64)).to(gpu))
        ck.append(torch.from_numpy(cast(kron, C64)).to(gpu))
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    n = V * color * ncols * spin
    x = int_vector(n)
    op = sb.create_kron_bsr(pi, dim, pd, dim, blk, blk, kr, kr, False, cii, cjj, cv, ck)
    dimx = [1, L, L, L, L, color, ncols, spin]
    half = [1, 2, L, L, L, color, ncols, spin]
    px = [([0, 2 * c, 0, 0, 0, 0, 0, 0], half) for c in range(2)]
    xs = x.reshape(2, n // 2)
    vx = [torch.from_numpy(xs[c].copy()).to(gpu) for c in range(2)]
    vy = [torch.full((n // 2,), 7.0, dtype=torch.complex128, device=gpu) for c in range(2)]
    ox, oy = ("pxyztcns", "pXYZTCnS") if adjoint else ("pXYZTCnS", "pxyztcns")
    try:
        sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", px, ox, [0] * 8, dimx, dimx, vx, 0.0, px, oy, [0] * 8,
                      dimx, dimx, "p", vy)
        torch.cuda.synchronize()
        kernel, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    finally:
        op.destroy()
    out = np.concatenate([v.cpu().numpy() for v in vy])
    A = lattice_case(L, color, color, spin, spin, False, False)[4]
    ref = (adjoint_ref if adjoint else forward_ref)(A, x, V, color, color, spin, spin, ncols)
    assert mixed == 1 and kernel == (15 if adjoint else 5 if ncols == 20 else 0)
    assert np.array_equal(out, ref)


def test_kron_mixed_host_component(gpu):
    """a host component (ii, jj, values and spin matrices in host memory): the owned device
    copies stay in the operator's type, 8 bytes per value"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 12
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, False, False, 2)
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    op = sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False, [torch.from_numpy(ii.copy())],
                            [torch.from_numpy(jj.copy())], [torch.from_numpy(cast(vals, C64))],
                            [torch.from_numpy(cast(kron, C64))])
    dimx = [1, L, L, L, L, color, ncols, spin]
    dimy = [2] + dimx[1:]
    tx, ty = torch.from_numpy(x.copy()).to(gpu), torch.from_numpy(y0.copy()).to(gpu)
    try:
        sb.bsr_krylov(ALPHA, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx, dimx,
                      [tx], BETA, [([0] * 8, dimy)], "pxyztcns", [0] * 8, dimy, dimy, "p", [ty])
        torch.cuda.synchronize()
        mixed = sb.tune_get("bsr.last_mixed")
    finally:
        op.destroy()
    assert mixed == 1 and np.array_equal(ty.cpu().numpy(), ref)


def sentinel(n, dtype):
    return np.full(n, 7.0, dtype)


@pytest.mark.parametrize("vt,xt,yt", [(C128, C64, C64), (C64, F64, F64), (C64, C128, C64), (C64, C64, C128),
                                      (F32, C128, C128), (F64, F32, F32)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_kron_mixed_refused_pairs(gpu, vt, xt, yt, adjoint):
    """with the key at 1 only float -> double and complex<float> -> complex<double> are admitted:
    a wider operator under narrower vectors, complex values under real vectors (and the
    reverse), x and y of different types keep raising, and y keeps its sentinel"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 2, 4, 3, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, vt)
    n = L ** 4 * color * ncols * spin
    dimx = [1, L, L, L, L, color, ncols, spin]
    tx = torch.from_numpy(cast(int_vector(n), xt)).to(gpu)
    ty = torch.from_numpy(sentinel(n, yt)).to(gpu)
    ox, oy = ("pxyztcns", "pXYZTCnS") if adjoint else ("pXYZTCnS", "pxyztcns")
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx, [tx],
                          0.0, [([0] * 8, dimx)], oy, [0] * 8, dimx, dimx, "p", [ty])
        torch.cuda.synchronize()
    finally:
        op.destroy()
    assert np.array_equal(ty.cpu().numpy(), sentinel(n, yt))


def test_kron_mixed_refused_half_values(gpu):
    """create_kron_bsr keeps refusing half-precision values with the key at 1"""
    import torch
    import superbblas_amd as sb
    from test_gpu_bsr_half import half_tensor
    L, spin, color = 2, 4, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    with pytest.raises(sb.SuperbblasError, match="unsupported type"):
        sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False,
                           [torch.from_numpy(ii).to(gpu)], [torch.from_numpy(jj).to(gpu)],
                           [half_tensor(vals.astype(C64), gpu)[0]],
                           [half_tensor(kron.astype(C64), gpu)[0]])


def test_kron_mixed_key_off_refuses_and_same_type_unchanged(gpu):
    """the key is read at each call: back at 0 the same handle is refused again (y untouched),
    and a same-type product of a complex<float> operator is the same with the key at 0 and 1"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 12
    ii, jj, vals, kron, x, y0, ref = forward_case(L, spin, color, ncols, False, False, 2)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    args = (sb, gpu, op, L, color, color, spin, spin, ncols, x)
    dimx = [1, L, L, L, L, color, ncols, spin]
    try:
        on = apply(*args, C128, ALPHA, BETA, y0, 2)
        same_on = apply(*args, C64, ALPHA, BETA, y0, 2)
        sb.tune_set("bsr.kron_mixed", 0)
        same_off = apply(*args, C64, ALPHA, BETA, y0, 2)
        ty = torch.from_numpy(sentinel(x.size, C128)).to(gpu)
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx, dimx,
                          [torch.from_numpy(x.copy()).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztcns", [0] * 8,
                          dimx, dimx, "p", [ty])
        torch.cuda.synchronize()
    finally:
        op.destroy()
    assert (on[0], on[1]) == (6, 1) and np.array_equal(on[2], ref)
    assert same_on[1] == 0 and same_off[1] == 0 and same_on[0] == same_off[0]
    assert np.array_equal(same_on[2], same_off[2]) and np.array_equal(same_on[2], ref)
    assert np.array_equal(ty.cpu().numpy(), sentinel(x.size, C128))


@functools.lru_cache(maxsize=None)
def random_case(L, ncols):
    """random complex<float> values and spin matrices, random complex<double> x"""
    rng = np.random.default_rng(29 + ncols)
    ii, jj, _, _ = kron_lattice(L, 4, 3)
    V = L ** 4
    vals = (rng.standard_normal(V * 81) + 1j * rng.standard_normal(V * 81)).astype(C64)
    kron = (rng.standard_normal(144) + 1j * rng.standard_normal(144)).astype(C64)
    x = rng.standard_normal(V * 12 * ncols) + 1j * rng.standard_normal(V * 12 * ncols)
    return ii, jj, vals, kron, x


@pytest.mark.parametrize("ncols", [12, 40])
def test_kron_mixed_deterministic(gpu, ncols):
    """two runs on random data are byte-identical"""
    import superbblas_amd as sb
    L, spin, color = 3, 4, 3
    ii, jj, vals, kron, x = random_case(L, ncols)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    try:
        a = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA)
        b = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128, ALPHA)
    finally:
        op.destroy()
    assert a[0] == b[0] == (6 if ncols == 12 else 5) and a[1] == 1
    assert a[2].tobytes() == b[2].tobytes() and np.abs(a[2]).max() > 0


def test_kron_mixed_random_values(gpu):
    """random data at 12 columns, componentwise against the oracle on the widened values:
    |y - ref| <= 128 * 2^-53 * (|K| |U| |x|), the right-hand side from the oracle on the absolute
    values -- a derived bound: 108 products and sums per output plus the alpha scaling, rounded
    up, each an FP64 operation on exactly widened operands"""
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 12
    V = L ** 4
    ii, jj, vals, kron, x = random_case(L, ncols)
    wide_v, wide_k = vals.astype(C128), kron.astype(C128)
    ref, mag = np.zeros_like(x), np.zeros_like(x)
    oracle_kron_bsr(T_CDOUBLE, [L, L, L, L, 1, 1], 0, V, 9, color, color, spin, spin, jj, wide_v, wide_k,
                    False, x, ref, ncols, 1.0)
    oracle_kron_bsr(T_CDOUBLE, [L, L, L, L, 1, 1], 0, V, 9, color, color, spin, spin, jj,
                    np.abs(wide_v).astype(C128), np.abs(wide_k).astype(C128), False,
                    np.abs(x).astype(C128), mag, ncols, 1.0)
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, C128)
    finally:
        op.destroy()
    bound = 128 * 2.0 ** -53 * mag.real
    err = np.abs(out - ref)
    print("kron mixed random: max err / bound %.3f" % (err / bound).max())
    assert (kernel, mixed) == (6, 1)
    assert np.all(err <= bound) and np.abs(ref).max() > 0
