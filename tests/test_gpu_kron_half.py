"""Half-precision Kronecker operators ("bsr.kron_half" 1): an operator of create_kron_bsr in
float16 / complex32 (IEEE binary16; colour blocks and spin matrices) applied by bsr_krylov to
float / complex<float> vectors, A x and A^H x.  Both arrays are read in place and widened exactly
at the load; products, sums, alpha, beta and y are FP32.  The references are the oracle's
double-precision product on the values widened from binary16 (test_gpu_kron_bsr.reference, or the
dense matrix of _kron_adjoint), and the comparisons are exact (np.array_equal).

Why exact: the data is integer valued (or integer multiples of one power of two, the quantum), and
each test establishes on the host that every partial sum stays below 2^24 quanta: it runs the
same oracle product on the absolute values (|re| + |im| of every operand, of alpha, beta and y0)
and asserts the maximum.  Every intermediate of the kernels, in whatever order, is bounded by
that product, so FP32 rounds nothing.  The kron_lattice data (|U| <= 5, |K| <= 4, |x| <= 8, 108
terms) meets the bound for one power, not for two; the power-2 cases take entries from
{0, +-1, +-i}.  Each case also asserts that its data survives the trip through binary16."""
import functools

import numpy as np
import pytest

from _kron_adjoint import adjoint_ref, dense_matrix, forward_ref, int_vector, lattice_case
from test_gpu_bsr_half import device_values, half_tensor, to_half, widened
from test_gpu_kron_bsr import kron_lattice, reference

pytestmark = pytest.mark.gpu

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
ALPHA, BETA = 1 - 1j, 2.0
EXACT = 2.0 ** 24
TYPES = [C64, F32]  # the vectors' type: complex32 under complex<float>, float16 under float


@pytest.fixture(autouse=True)
def kron_half_on(gpu):
    """the key at 1 for the test, put back afterwards"""
    import superbblas_amd as sb
    old = sb.tune_get("bsr.kron_half")
    sb.tune_set("bsr.kron_half", 1)
    yield
    sb.tune_set("bsr.kron_half", old)


def cast(a, dtype):
    return np.ascontiguousarray(a.astype(dtype) if np.dtype(dtype).kind == "c" else a.real.astype(dtype))


def mag(a):
    """|re| + |im| of every element (of a scalar too), as complex128"""
    a = np.asarray(a, C128)
    return (np.abs(a.real) + np.abs(a.imag)).astype(C128)


def alpha_of(xt):
    return ALPHA if xt == C64 else 2.0


def through_half(a, xt):
    """the array in the vectors' type; asserts that binary16 holds it unchanged"""
    w = cast(a, xt)
    assert np.array_equal(widened(to_half(w), xt == C64), w)
    return w


def unit_entries(a):
    """entries from {0, +-1, +-i} where a is nonzero (a's zero pattern is kept)"""
    table = np.array([1, -1, 1j, -1j, 0, 1, 1j, -1, -1j, 1, 0], C128)
    return table[np.arange(a.size) % table.size] * (a != 0)


def make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, xt, lead=0):
    """(operator, value tensor, its float16 view, spin-matrix tensor): values and spin matrices
    in binary16 (asserted exact); lead: both tensors start that many elements into their buffers"""
    import torch
    cplx = xt == C64
    dimi, dimd = [L, L, L, L, ki, bi], [L, L, L, L, kd, bd]
    tv, tv16 = device_values(to_half(through_half(vals, xt)), cplx, gpu, lead)
    tk, _ = device_values(to_half(through_half(kron, xt)), cplx, gpu, lead)
    assert tv.dtype == tk.dtype == (torch.complex32 if cplx else torch.float16)
    op = sb.create_kron_bsr([([0] * 6, dimi)], dimi, [([0] * 6, dimd)], dimd,
                            [1, 1, 1, 1, 1, bi], [1, 1, 1, 1, 1, bd], [1, 1, 1, 1, ki, 1],
                            [1, 1, 1, 1, kd, 1], bif, [torch.from_numpy(np.array(ii)).to(gpu)],
                            [torch.from_numpy(np.array(jj)).to(gpu)], [tv], [tk])
    return op, tv, tv16, tk


def apply(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, xt, alpha=1.0, beta=0.0, y0=None, power=1,
          adjoint=False, **kw):
    """forward: y (pxyztcns) = alpha A^(p+1) x (pXYZTCnS) + beta y0; adjoint: the labels swapped.
    Vectors in xt.  Returns (last_kernel, last_mixed, y as complex128)"""
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


@functools.lru_cache(maxsize=None)
def forward_case(L, ncols, bif, sparse, power, real, unit=False):
    """(ii, jj, vals, kron, x, y0, reference) of the 3x3 (x) 4x4 9-point lattice, computed once and
    shared; the exactness bound is asserted here.  unit: entries from {0, +-1, +-i} and |x| <= 2"""
    spin, color = 4, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color, sparse_kron=sparse)
    vals, kron = vals.astype(C128), kron.astype(C128)
    n = L ** 4 * color * ncols * spin
    g = np.arange(n)
    x = ((g % 5 - 2) + 1j * (g % 3 - 1)).astype(C128)
    y0 = ((np.arange(n * power) % 7 - 3) + 1j).astype(C128)
    if unit:
        vals, kron = unit_entries(vals), unit_entries(kron)
        x = ((g % 3 - 1) + 1j * (g % 2)).astype(C128)
    if real:
        vals, kron, x, y0 = (a.real.astype(C128) for a in (vals, kron, x, y0))
    alpha = 2.0 if real else ALPHA
    ref = reference(L, spin, color, ncols, vals, kron, jj, x, alpha, BETA, y0, power, bif)
    top = reference(L, spin, color, ncols, mag(vals), mag(kron), jj, mag(x), mag(alpha), BETA, mag(y0),
                    power, bif)
    assert top.real.max() < EXACT, top.real.max()
    assert np.abs(ref).max() > 0
    for a in (ii, jj, vals, kron, x, y0, ref):
        a.setflags(write=False)
    return ii, jj, vals, kron, x, y0, ref


def run_forward(gpu, L, ncols, bif, sparse, power, xt, unit=False, lead=0):
    import superbblas_amd as sb
    ii, jj, vals, kron, x, y0, ref = forward_case(L, ncols, bif, sparse, power, xt == F32, unit)
    op, tv, _, tk = make_op(sb, gpu, L, 3, 3, 4, 4, bif, ii, jj, vals, kron, xt, lead)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, 3, 3, 4, 4, ncols, x, xt, alpha_of(xt), BETA, y0, power)
    finally:
        op.destroy()
    assert (kernel, mixed) == (0, 1), (kernel, mixed)
    assert np.array_equal(out, ref)
    return tv, tk


# (ncols, L).  L = 3: 81 sites, a last workgroup with fewer rows than its slots.  1 and 3:
# bsr_kron_kernel; from 4 bsr_kron_lds_kernel with S = 256 / ncols rows a workgroup: 4 S = 64;
# 5, 10 and 17 an odd S (51, 25, 15), where S * 81 two-byte values end 2 mod 4 and the block
# columns behind them need the pad; 300 at L = 2: two column groups of 256 and 44
FORWARD = [(1, 3), (3, 3), (4, 3), (5, 3), (10, 3), (17, 3), (12, 3), (40, 3), (300, 2)]


@pytest.mark.parametrize("ncols,L", FORWARD)
@pytest.mark.parametrize("bif,sparse", [(False, False), (True, True)])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_forward(gpu, xt, bif, sparse, ncols, L):
    """complex32 under complex<float> and float16 under float, 3x3 (x) 4x4, complex alpha (real
    vectors: 2), beta 2 and a non-zero y0: both VALU forms give the reference, bit for bit"""
    run_forward(gpu, L, ncols, bif, sparse, 1, xt)


@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_forward_power2(gpu, xt):
    """two powers (entries from {0, +-1, +-i}: the second power's sums stay below 2^24)"""
    run_forward(gpu, 3, 12, False, False, 2, xt, unit=True)


@functools.lru_cache(maxsize=None)
def dense_case(L, bi, bd, ki, kd, sparse, bif, real):
    """lattice_case and the dense matrix of the absolute values (the bound's operator)"""
    ii, jj, vals, kron, A = lattice_case(L, bi, bd, ki, kd, sparse, bif, real)
    top = dense_matrix(L, bi, bd, ki, kd, jj, mag(vals), mag(kron), bif)
    top.setflags(write=False)
    return ii, jj, vals, kron, A, top


def dense_run(gpu, L, bi, bd, ki, kd, sparse, bif, xt, ncols, adjoint, kernel_want, alpha=1.0, beta=0.0):
    """one product against the dense matrix, the bound asserted from the dense matrix of the
    absolute values"""
    import superbblas_amd as sb
    real = xt == F32
    V = L ** 4
    ii, jj, vals, kron, A, top = dense_case(L, bi, bd, ki, kd, sparse, bif, real)
    nx = V * (bi * ki if adjoint else bd * kd) * ncols
    ny = V * (bd * kd if adjoint else bi * ki) * ncols
    x = int_vector(nx, cplx=not real, seed=3 if not adjoint else 0)
    y0 = ((np.arange(ny) % 7 - 3) + (0 if real else 1j)).astype(C128)
    ref_of = adjoint_ref if adjoint else forward_ref
    dims = (V, bi, bd, ki, kd, ncols)
    ref = alpha * ref_of(A, x, *dims) + beta * y0
    bound = mag(alpha) * ref_of(top, mag(x), *dims) + abs(beta) * mag(y0)
    assert bound.real.max() < EXACT and np.abs(ref).max() > 0
    op, _, _, _ = make_op(sb, gpu, L, bi, bd, ki, kd, bif, ii, jj, vals, kron, xt)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, bi, bd, ki, kd, ncols, x, xt, alpha, beta, y0,
                                   adjoint=adjoint)
    finally:
        op.destroy()
    assert (kernel, mixed) == (kernel_want, 1), (kernel, mixed)
    assert out.size == ny and np.array_equal(out, ref)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_generic_sizes(gpu, xt, adjoint):
    """colour 2 (x) spin 2: the generic kernels (19 for the mixed generic adjoint)"""
    dense_run(gpu, 3, 2, 2, 2, 2, False, False, xt, 3, adjoint, 19 if adjoint else 0, alpha_of(xt), BETA)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("bif", [False, True])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_rectangular(gpu, xt, bif, adjoint):
    """ki != kd and bi != bd (Kronecker matrices 2 x 4, blocks 3 x 2, half of every spin matrix
    zero): A x and A^H x on the generic kernels, a swapped index does not cancel out"""
    dense_run(gpu, 2, 3, 2, 2, 4, True, bif, xt, 3, adjoint, 19 if adjoint else 0)


# 1, 5, 12 and 31 columns: a lane reads its blocks itself; 32 and 40 (KRON_ADJ_STAGE_COLS on): the
# blocks staged in LDS, widened there
@pytest.mark.parametrize("ncols", [1, 5, 12, 31, 32, 40])
@pytest.mark.parametrize("bif,sparse", [(False, False), (True, True)])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_adjoint(gpu, xt, bif, sparse, ncols):
    """A^H, both types, 3x3 (x) 4x4 on 81 sites: bsr_kron_adj_kernel in both forms, complex alpha,
    beta 2, against the dense matrix"""
    dense_run(gpu, 3, 3, 3, 4, 4, sparse, bif, xt, ncols, True, 15, alpha_of(xt), BETA)


@pytest.mark.parametrize("ncols", [5, 12])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_alignment_forward(gpu, xt, ncols):
    """the value tensor and the spin tensor start one element into their buffers (complex32 only
    4-byte aligned, float16 only 2-byte aligned) and the buffers end with the arrays' last
    elements; 5 and 12 columns stage the values through LDS (5: odd S)"""
    tv, tk = run_forward(gpu, 3, ncols, False, False, 1, xt, lead=1)
    es = 4 if xt == C64 else 2
    assert tv.data_ptr() % (2 * es) == es and tk.data_ptr() % (2 * es) == es
    assert tv.numel() == 81 * 81 and tk.numel() == 144


@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_alignment_adjoint(gpu, xt):
    """the same tensors under A^H at 32 columns (the staged form)"""
    import superbblas_amd as sb
    L, ncols, real = 3, 32, xt == F32
    V = L ** 4
    ii, jj, vals, kron, A, top = dense_case(L, 3, 3, 4, 4, False, False, real)
    x = int_vector(V * 12 * ncols, cplx=not real)
    dims = (V, 3, 3, 4, 4, ncols)
    assert adjoint_ref(top, mag(x), *dims).real.max() < EXACT
    op, tv, _, tk = make_op(sb, gpu, L, 3, 3, 4, 4, False, ii, jj, vals, kron, xt, lead=1)
    es = 4 if xt == C64 else 2
    assert tv.data_ptr() % (2 * es) == es and tk.data_ptr() % (2 * es) == es
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, 3, 3, 4, 4, ncols, x, xt, adjoint=True)
    finally:
        op.destroy()
    assert (kernel, mixed) == (15, 1)
    assert np.array_equal(out, adjoint_ref(A, x, *dims))


# binary16 edge values, as multiples of a quantum: subnormals (k * 2^-24, k < 1024), the smallest
# normal and +-0; the largest finite value 65504 = 2047 * 32 and powers of two from 32
SUBNORMAL = (np.array([0.0, -0.0, 1, -1, 2, 3, -5, 1023, -1023, 7, 1024, -512]) * 2.0 ** -24, 2.0 ** -24)
LARGEST = (np.array([65504.0, -65504.0, 32, -64, 1024, 32768, -32768, 2048, 0.0, 16384, -65504.0]), 32.0)


@functools.lru_cache(maxsize=None)
def edge_case(which, real):
    """(ii, jj, vals, kron, A, the abs-value matrix) on a 2^4 lattice: colour entries from the
    table, spin entries from {0, +-1, +-i}"""
    L = 2
    table, _ = (SUBNORMAL, LARGEST)[which]
    ii, jj, v0, k0 = kron_lattice(L, 4, 3)
    k = np.arange(v0.size)
    vals = np.empty(v0.size, C128)  # (filled part by part: -0 keeps its sign)
    vals.real, vals.imag = table[k % table.size], table[(3 * k + 1) % table.size]
    kron = unit_entries(k0.astype(C128))
    if real:
        vals, kron = vals.real.astype(C128), kron.real.astype(C128)
    A = dense_matrix(L, 3, 3, 4, 4, jj, vals, kron, False)
    top = dense_matrix(L, 3, 3, 4, 4, jj, mag(vals), mag(kron), False)
    return ii, jj, vals, kron, A, top


@pytest.mark.parametrize("ncols,adjoint", [(3, False), (12, False), (12, True), (32, True)])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_edge_values(gpu, xt, which, ncols, adjoint):
    """subnormal halves and +-0, then +-65504 and powers of two, under x of small powers of two:
    every operand is a multiple of its quantum and the absolute-value product stays below 2^24
    quanta, so the FP32 result is exact -- if the widening is (subnormals, the largest value)"""
    import superbblas_amd as sb
    L, real = 2, xt == F32
    V = L ** 4
    ii, jj, vals, kron, A, top = edge_case(which, real)
    quantum = (SUBNORMAL, LARGEST)[which][1] * 0.5  # (the colour quantum) x (x's smallest: 1/2)
    g = np.arange(V * 12 * ncols)
    pw = np.array([0.5, 1, 2, -1, -0.5, 2, 1, -2])
    x = (pw[g % 8] + (0 if real else 1j) * pw[(3 * g + 2) % 8]).astype(C128)
    dims = (V, 3, 3, 4, 4, ncols)
    ref_of = adjoint_ref if adjoint else forward_ref
    ref = ref_of(A, x, *dims)
    assert np.array_equal(np.round(ref / quantum) * quantum, ref)  # multiples of the quantum
    assert ref_of(top, mag(x), *dims).real.max() / quantum < EXACT and np.abs(ref).max() > 0
    # (the table's entries as binary16: subnormals and -0 are among them; make_op asserts the trip)
    h16 = to_half(cast(vals, xt))
    if which == 0:
        assert np.any((h16 != 0) & (np.abs(h16) < 2.0 ** -14)) and np.any(np.signbit(h16) & (h16 == 0))
    else:
        assert np.any(np.abs(h16) == 65504)
    op, _, _, _ = make_op(sb, gpu, L, 3, 3, 4, 4, False, ii, jj, vals, kron, xt)
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, 3, 3, 4, 4, ncols, x, xt, adjoint=adjoint)
    finally:
        op.destroy()
    assert (kernel, mixed) == (15 if adjoint else 0, 1)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_values_in_place(gpu, xt):
    """no snapshot and no widened copy: after the caller doubles the values through the tensor's
    float16 view (exact), A x and A^H x of the same handle are those of the doubled operator"""
    import superbblas_amd as sb
    L, ncols, real = 2, 12, xt == F32
    V = L ** 4
    ii, jj, vals, kron, A, top = dense_case(L, 3, 3, 4, 4, False, False, real)
    x = int_vector(V * 12 * ncols, cplx=not real)
    dims = (V, 3, 3, 4, 4, ncols)
    assert 2 * max(forward_ref(top, mag(x), *dims).real.max(), adjoint_ref(top, mag(x), *dims).real.max()) < EXACT
    through_half(2 * vals, xt)
    op, tv, tv16, _ = make_op(sb, gpu, L, 3, 3, 4, 4, False, ii, jj, vals, kron, xt)
    args = (sb, gpu, op, L, 3, 3, 4, 4, ncols, x, xt)
    try:
        f1, a1 = apply(*args)[2], apply(*args, adjoint=True)[2]
        tv16.mul_(2)
        f2, a2 = apply(*args)[2], apply(*args, adjoint=True)[2]
    finally:
        op.destroy()
    rf, ra = forward_ref(A, x, *dims), adjoint_ref(A, x, *dims)
    assert np.abs(rf).max() > 0 and np.abs(ra).max() > 0
    assert np.array_equal(f1, rf) and np.array_equal(a1, ra)
    assert np.array_equal(f2, 2 * rf) and np.array_equal(a2, 2 * ra)


@pytest.mark.parametrize("adjoint", [False, True])
def test_kron_half_two_components_halo(gpu, adjoint):
    """one process, two components on one device: A's image split in two along x on a 4^4 lattice,
    each component's domain its image plus a one-site halo in every direction (the split of
    test_gpu_kron_mixed.test_kron_mixed_two_components_halo).  A x at power 2, entries from
    {0, +-1, +-i}: the first power reaches the second through the halo exchange in complex<float>.
    A^H x at one power: the components' contributions to one domain site are summed"""
    import torch
    import superbblas_amd as sb
    from _kron_adjoint import DIRS
    L, spin, color, ncols, xt = 4, 4, 3, 12, C64
    power = 1 if adjoint else 2
    V = L ** 4
    n = V * color * ncols * spin
    if adjoint:
        ii, jj, vals, kron, A, top = dense_case(L, color, color, spin, spin, False, False, False)
        x = int_vector(n)
        dims = (V, color, color, spin, spin, ncols)
        ref = adjoint_ref(A, x, *dims)
        assert adjoint_ref(top, mag(x), *dims).real.max() < EXACT
    else:
        ii, jj, v0, k0 = kron_lattice(L, spin, color)
        vals, kron = unit_entries(v0.astype(C128)), unit_entries(k0.astype(C128))
        g = np.arange(n)
        x = ((g % 3 - 1) + 1j * (g % 2)).astype(C128)
        zero = np.zeros(n * power, C128)
        ref = reference(L, spin, color, ncols, vals, kron, jj, x, 1.0, 0.0, zero, power)
        top = reference(L, spin, color, ncols, mag(vals), mag(kron), jj, mag(x), 1.0, 0.0, zero, power)
        assert top.real.max() < EXACT
    assert np.abs(ref).max() > 0
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
    allv = through_half(vals, xt).reshape(V, 9 * color * color)
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
        cv.append(half_tensor(np.ascontiguousarray(allv[gsite]).ravel(), gpu)[0])
        ck.append(half_tensor(through_half(kron, xt), gpu)[0])
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    op = sb.create_kron_bsr(pi, dim, pd, dim, blk, blk, kr, kr, False, cii, cjj, cv, ck)
    dimx = [1, L, L, L, L, color, ncols, spin]
    dimy = [power] + dimx[1:]
    halfx = [1, 2, L, L, L, color, ncols, spin]
    halfy = [power] + halfx[1:]
    px = [([0, 2 * c, 0, 0, 0, 0, 0, 0], halfx) for c in range(2)]
    py = [([0, 2 * c, 0, 0, 0, 0, 0, 0], halfy) for c in range(2)]
    xs = cast(x, xt).reshape(2, n // 2)
    vx = [torch.from_numpy(xs[c].copy()).to(gpu) for c in range(2)]
    vy = [torch.full((power * n // 2,), 7.0, dtype=torch.complex64, device=gpu) for c in range(2)]
    ox, oy = ("pxyztcns", "pXYZTCnS") if adjoint else ("pXYZTCnS", "pxyztcns")
    try:
        sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", px, ox, [0] * 8, dimx, dimx, vx, 0.0, py, oy, [0] * 8,
                      dimy, dimy, "p", vy)
        torch.cuda.synchronize()
        kernel, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    finally:
        op.destroy()
    # each component holds (power, its half of x, ...): back to (power, the whole lattice, ...)
    out = np.concatenate([v.cpu().numpy().reshape(power, n // 2) for v in vy], axis=1).ravel().astype(C128)
    assert (kernel, mixed) == (15 if adjoint else 0, 1)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_host_component(gpu, xt):
    """a host component (ii, jj, values and spin matrices host arrays of binary16): the owned
    device copies are byte for byte, 4 / 2 bytes per value"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols, cplx = 3, 4, 3, 12, xt == C64
    ii, jj, vals, kron, x, y0, ref = forward_case(L, ncols, False, False, 1, not cplx)
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    t16 = [torch.from_numpy(to_half(through_half(a, xt))) for a in (vals, kron)]
    tv, tk = [torch.view_as_complex(t.view(-1, 2)) if cplx else t for t in t16]
    assert not tv.is_cuda and not tk.is_cuda and tv.numel() == vals.size
    op = sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False, [torch.from_numpy(ii.copy())],
                            [torch.from_numpy(jj.copy())], [tv], [tk])
    try:
        kernel, mixed, out = apply(sb, gpu, op, L, color, color, spin, spin, ncols, x, xt, alpha_of(xt), BETA,
                                   y0)
    finally:
        op.destroy()
    assert (kernel, mixed) == (0, 1) and np.array_equal(out, ref)


def sentinel(n, dtype):
    return np.full(n, 7.0, dtype)


@pytest.mark.parametrize("vt,xt", [(C64, C128), (F32, F64), (F32, C64), (C64, F32)])
@pytest.mark.parametrize("adjoint", [False, True])
def test_kron_half_refused_pairs(gpu, vt, xt, adjoint):
    """with the key at 1 only float16 -> float and complex32 -> complex<float> are admitted: a
    half Kronecker handle under double vectors, a float16 one under complex<float> vectors and a
    complex32 one under float vectors keep raising, and y keeps its sentinel"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 2, 4, 3, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    op, _, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, vt)
    n = L ** 4 * color * ncols * spin
    dimx = [1, L, L, L, L, color, ncols, spin]
    tx = torch.from_numpy(cast(int_vector(n), xt)).to(gpu)
    ty = torch.from_numpy(sentinel(n, xt)).to(gpu)
    ox, oy = ("pxyztcns", "pXYZTCnS") if adjoint else ("pXYZTCnS", "pxyztcns")
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx, [tx],
                          0.0, [([0] * 8, dimx)], oy, [0] * 8, dimx, dimx, "p", [ty])
        torch.cuda.synchronize()
    finally:
        op.destroy()
    assert np.array_equal(ty.cpu().numpy(), sentinel(n, xt))


@pytest.mark.parametrize("xt", TYPES)
def test_kron_half_refused_half_vectors(gpu, xt):
    """half vectors stay refused (no tensor has a half type), y keeps its sentinel"""
    import superbblas_amd as sb
    L, spin, color, ncols = 2, 4, 3, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    op, _, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, xt)
    n = L ** 4 * color * ncols * spin
    dimx = [1, L, L, L, L, color, ncols, spin]
    tx, _ = half_tensor(cast(int_vector(n), xt), gpu)
    ty, ty16 = half_tensor(sentinel(n, xt), gpu)
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx, dimx,
                          [tx], 0.0, [([0] * 8, dimx)], "pxyztcns", [0] * 8, dimx, dimx, "p", [ty])
    finally:
        op.destroy()
    assert np.array_equal(ty16.cpu().numpy(), to_half(sentinel(n, xt)))


def test_kron_half_key_off(gpu):
    """the key is read at each call: back at 0 the same handle is refused at bsr_krylov with the
    handle-mismatch error (y untouched) and create_kron_bsr throws "unsupported type" again
    (whatever bsr.kron_mixed); a same-type complex<float> Kronecker product is byte-identical
    with the key at 0 and at 1"""
    import torch
    import superbblas_amd as sb
    L, spin, color, ncols = 3, 4, 3, 12
    ii, jj, vals, kron, x, y0, ref = forward_case(L, ncols, False, False, 1, False)
    op, _, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron, C64)
    args = (L, color, color, spin, spin, ncols, x, C64, ALPHA, BETA, y0)
    dimx = [1, L, L, L, L, color, ncols, spin]
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    same = sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False,
                              [torch.from_numpy(ii.copy()).to(gpu)], [torch.from_numpy(jj.copy()).to(gpu)],
                              [torch.from_numpy(cast(vals, C64)).to(gpu)],
                              [torch.from_numpy(cast(kron, C64)).to(gpu)])
    old_mixed = sb.tune_get("bsr.kron_mixed")
    try:
        on = apply(sb, gpu, op, *args)
        same_on = apply(sb, gpu, same, *args)
        sb.tune_set("bsr.kron_half", 0)
        same_off = apply(sb, gpu, same, *args)
        ty = torch.from_numpy(sentinel(x.size, C64)).to(gpu)
        with pytest.raises(sb.SuperbblasError, match="doesn't match the template parameters"):
            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx, dimx,
                          [torch.from_numpy(cast(x, C64)).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztcns", [0] * 8,
                          dimx, dimx, "p", [ty])
        torch.cuda.synchronize()
        for km in (0, 1):
            sb.tune_set("bsr.kron_mixed", km)
            with pytest.raises(sb.SuperbblasError, match="unsupported type"):
                sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False,
                                   [torch.from_numpy(ii.copy()).to(gpu)], [torch.from_numpy(jj.copy()).to(gpu)],
                                   [half_tensor(cast(vals, C64), gpu)[0]], [half_tensor(cast(kron, C64), gpu)[0]])
    finally:
        sb.tune_set("bsr.kron_mixed", old_mixed)
        op.destroy()
        same.destroy()
    assert (on[0], on[1]) == (0, 1) and np.array_equal(on[2], ref)
    assert same_on[1] == 0 and same_off[1] == 0 and same_on[0] == same_off[0]
    assert same_on[2].tobytes() == same_off[2].tobytes() and np.array_equal(same_on[2], ref)
    assert np.array_equal(ty.cpu().numpy(), sentinel(x.size, C64))


@functools.lru_cache(maxsize=None)
def random_case(L, ncols, adjoint):
    """random values in [-1, 1] rounded to binary16 on the host (widened back: what the kernels
    read), random complex<float> x; the oracle's product and its absolute-value product"""
    rng = np.random.default_rng(31 + ncols)
    ii, jj, _, _ = kron_lattice(L, 4, 3)
    V = L ** 4
    rnd = lambda n: (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(C64)
    vals = widened(to_half(rnd(V * 81)), True).astype(C128)
    kron = widened(to_half(rnd(144)), True).astype(C128)
    x = rnd(V * 12 * ncols).astype(C128)
    if adjoint:
        dims = (V, 3, 3, 4, 4, ncols)
        ref = adjoint_ref(dense_matrix(L, 3, 3, 4, 4, jj, vals, kron, False), x, *dims)
        top = adjoint_ref(dense_matrix(L, 3, 3, 4, 4, jj, mag(vals), mag(kron), False), mag(x), *dims)
    else:
        zero = np.zeros_like(x)
        ref = reference(L, 4, 3, ncols, vals, kron, jj, x, 1.0, 0.0, zero, 1)
        top = reference(L, 4, 3, ncols, mag(vals), mag(kron), jj, mag(x), 1.0, 0.0, zero, 1)
    return ii, jj, vals, kron, x, ref, top.real


@pytest.mark.parametrize("ncols", [12, 40])
@pytest.mark.parametrize("adjoint", [False, True])
def test_kron_half_random_deterministic(gpu, ncols, adjoint):
    """random data at L = 3: two runs are byte-identical, and the result agrees componentwise with
    the oracle on the widened values, |y - ref| <= 128 * 2^-24 * top per real and imaginary part,
    top the oracle's product of the absolute values (|re| + |im| of every operand: it dominates the
    sum of the absolute real triple products behind either part).  Derived from the roundings on
    the longest path of one term into its output, operands exact (x is FP32 data, the values are
    widened exactly).  A x: the spin sum over b (4 complex FMAs: a product and 8 additions), the
    colour product and its sum over d and the 9 neighbours (a product and 54 additions), alpha = 1:
    64 roundings.  A^H x: the colour sum over i (a product, 6 additions), the spin sum over a and
    the site's 9 entries (a product, 72 additions): 80.  Each is relative 2^-24 on a partial sum
    bounded by top: gamma_80 = 80 * 2^-24 / (1 - 80 * 2^-24) < 128 * 2^-24 (fused multiply-adds
    only remove roundings)"""
    import superbblas_amd as sb
    L = 3
    ii, jj, vals, kron, x, ref, top = random_case(L, ncols, adjoint)
    op, _, _, _ = make_op(sb, gpu, L, 3, 3, 4, 4, False, ii, jj, vals, kron, C64)
    try:
        a = apply(sb, gpu, op, L, 3, 3, 4, 4, ncols, x, C64, adjoint=adjoint)
        b = apply(sb, gpu, op, L, 3, 3, 4, 4, ncols, x, C64, adjoint=adjoint)
    finally:
        op.destroy()
    assert a[0] == b[0] == (15 if adjoint else 0) and a[1] == b[1] == 1
    assert a[2].tobytes() == b[2].tobytes() and np.abs(a[2]).max() > 0
    bound = 128 * 2.0 ** -24 * top
    err = np.maximum(np.abs((a[2] - ref).real), np.abs((a[2] - ref).imag))
    print("kron half random (%d columns, adjoint %d): max err / bound %.4f" % (ncols, adjoint, (err / bound).max()))
    assert np.all(err <= bound) and np.abs(ref).max() > 0
