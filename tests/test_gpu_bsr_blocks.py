"""bsr_blk_mfma_kernel (kernels_bsr.hip), its same-type form: dense blocks of 16 x 16 and more --
the multigrid coarse operators -- on the matrix cores, "bsr.last_kernel" 14.  Exact against the oracle's builtin
BSR loop (bsr.h:535-650) on integer-valued data: components are at most 6, a product component
at most 61 and a row sum at most 9 * 128 * 61 = 70 272 < 2^24, so every sum is exact in float32
in any order.  Small lattices: (2,2,2,2) has 16 rows of five blocks, (1,3,1,5) 15 rows of five
and (3,2,1,3) 18 rows of six."""
import numpy as np
import pytest

from _common import TYPE_OF, int_valued, oracle_bsr, oracle_bsr_adjoint, random_valued, stencil_jj

pytestmark = pytest.mark.gpu

FORM = 14
LAT = (2, 2, 2, 2)


def split(b):
    """the block size as spin x color"""
    return (2, b // 2) if b % 2 == 0 else (1, b)


def stencil(lat):
    """Nonzero block sites of the periodic stencil of test_gpu_bsr.lattice_operator on any
    lattice: the site, then per direction its -1 and +1 neighbours (one for an extent of 2, none
    for 1); [vol, nb, 4] coordinates."""
    vol = int(np.prod(lat))
    sites = np.array(np.unravel_index(np.arange(vol), lat)).T
    nbrs = [sites]
    for d in range(4):
        for dr in ((-1, 1) if lat[d] > 2 else (-1,) if lat[d] == 2 else ()):
            c = sites.copy()
            c[:, d] = (c[:, d] + dr) % lat[d]
            nbrs.append(c)
    return np.stack(nbrs, axis=1)


class Op:
    """A stencil operator with bi x bd blocks and integer values; jj may be edited before create()"""

    def __init__(self, lat, bi, bd, dtype, seed=1, values=int_valued):
        self.lat, self.bi, self.bd, self.dtype = list(lat), bi, bd, np.dtype(dtype)
        self.vol = int(np.prod(lat))
        self.sites = stencil(lat)
        self.nb = self.sites.shape[1]
        self.dimi = self.lat + list(split(bi))
        self.dimd = self.lat + list(split(bd))
        self.ii = np.full(self.vol, self.nb, np.int32)
        self.jj = np.concatenate([self.sites, np.zeros((self.vol, self.nb, 2), np.int64)],
                                 axis=2).astype(np.int32).reshape(-1, 6)
        self.vals = values(self.vol * self.nb * bi * bd, dtype, seed)

    def keep(self, counts):
        """row r keeps its first counts[r] blocks (a CSR operator)"""
        sel = np.concatenate([np.arange(r * self.nb, r * self.nb + counts[r], dtype=np.int64)
                              for r in range(self.vol)])
        self.ii = np.asarray(counts, np.int32)
        self.jj = np.ascontiguousarray(self.jj[sel])
        self.vals = np.ascontiguousarray(self.vals.reshape(-1, self.bi * self.bd)[sel]).reshape(-1)

    def create(self, gpu, im_fast=False):
        import torch
        import superbblas_amd as sb
        pi, pd = [([0] * 6, self.dimi)], [([0] * 6, self.dimd)]
        return sb.create_bsr(pi, self.dimi, pd, self.dimd, [1, 1, 1, 1] + list(split(self.bi)),
                             [1, 1, 1, 1] + list(split(self.bd)), im_fast,
                             [torch.from_numpy(self.ii).to(gpu)],
                             [torch.from_numpy(self.jj.reshape(-1)).to(gpu)],
                             [torch.from_numpy(self.vals).to(gpu)])


def layout(lat, b, ncols, row, upper):
    """(order, dim) of a right-hand side: row major (columns fastest) or column major"""
    o = "XYZTSC" if upper else "xyztsc"
    if row:
        return "p" + o + "n", [1] + list(lat) + list(split(b)) + [ncols]
    return "pn" + o, [1, ncols] + list(lat) + list(split(b))


def apply(gpu, op, h, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, adjoint=False):
    """y = alpha A x + beta y0 (A^H x when adjoint: x carries the image labels); returns y on the
    host and the kernel form"""
    import torch
    import superbblas_amd as sb
    bx, by = (op.bi, op.bd) if adjoint else (op.bd, op.bi)
    ox, dimx = layout(op.lat, bx, ncols, xrow, not adjoint)
    oy, dimy = layout(op.lat, by, ncols, yrow, adjoint)
    ty = torch.from_numpy(y0.copy()).to(gpu)
    sb.bsr_krylov(alpha, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], beta, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                  "p", [ty])
    torch.cuda.synchronize()
    return ty.cpu().numpy(), sb.tune_get("bsr.last_kernel")


def reference(op, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, im_fast=False):
    y = (beta * y0).astype(op.dtype)
    oracle_bsr(TYPE_OF[op.dtype], op.dimd, 0, op.vol, op.bi, op.bd, op.ii, op.jj.reshape(-1),
               op.vals, im_fast, x, ncols if xrow else op.vol * op.bd, xrow, y,
               ncols if yrow else op.vol * op.bi, yrow, ncols, alpha, add=True)
    return y


def sentinel(n, dtype):
    return np.full(n, 7.0, dtype)


C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
# a pairwise-covering subset of (block) x (type) x (columns) x (x layout) x (y layout) x
# (block_im_fast): every listed value of every axis, every type with a block that is no multiple
# of 16 and a partial column tile.  (The default dispatch takes blocks of fewer than 1024
# elements from 4 rhs columns and of fewer than 576 from 12: the small blocks come with such counts.)
EXACT = [
    (16, 16, C64, 16, True, True, False), (16, 16, F32, 300, False, True, True),
    (24, 24, C128, 12, True, False, False), (24, 24, F64, 17, False, False, True),
    (24, 24, C64, 300, True, True, False), (48, 48, C64, 12, True, True, False),
    (48, 48, C128, 3, True, True, True), (48, 48, F32, 40, True, False, False),
    (64, 64, C64, 16, True, True, False), (64, 64, C128, 40, False, True, False),
    (64, 64, F64, 1, True, True, True), (20, 36, C64, 17, False, False, True),
    (20, 36, C128, 12, True, True, False), (20, 36, F32, 40, True, True, False),
    (18, 22, C64, 17, True, False, False), (18, 22, F32, 12, True, True, False),
    (18, 22, F64, 40, False, True, True), (18, 22, C128, 12, False, False, False),
    (32, 16, C64, 40, True, True, True), (32, 16, F64, 12, True, True, False),
    (16, 80, C128, 17, True, True, False), (16, 80, F32, 16, False, False, False),
    (96, 96, C64, 3, True, True, False), (96, 96, F64, 17, True, True, True),
    (128, 128, C128, 12, True, True, False), (128, 128, C64, 17, False, True, True),
    (128, 128, F32, 1, True, False, True),
]


@pytest.mark.parametrize("bi,bd,dtype,ncols,xrow,yrow,imf", EXACT)
def test_blocks_exact(gpu, bi, bd, dtype, ncols, xrow, yrow, imf):
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols, xrow, yrow, im_fast=imf)
    h = op.create(gpu, imf)
    y, form = apply(gpu, op, h, x, y0, ncols, xrow, yrow)
    h.destroy()
    assert form == FORM, form
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd,dtype", [(48, 48, C64), (20, 36, F64)])
@pytest.mark.parametrize("alpha,beta", [(2 - 1j, 1.0), (-1.0, 0.0)])
def test_blocks_alpha_beta(gpu, bi, bd, dtype, alpha, beta):
    ncols = 5
    if np.dtype(dtype).kind != "c":
        alpha = alpha.real
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = int_valued(op.vol * bi * ncols, dtype, 3)
    ref = reference(op, x, y0, ncols, alpha=alpha, beta=beta)
    h = op.create(gpu)
    y, form = apply(gpu, op, h, x, y0, ncols, alpha=alpha, beta=beta)
    h.destroy()
    assert form == FORM, form
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pattern", ["ragged", "skipped"])
@pytest.mark.parametrize("bi,bd,dtype,ncols", [(48, 48, C64, 13), (48, 48, C64, 16),
                                               (20, 36, C128, 5)])
def test_blocks_ragged_and_skipped(gpu, bi, bd, dtype, ncols, pattern):
    """create_bsr takes blocks with column -1 only where every row has the same number of blocks
    (as the reference, bsr.h:1424-1468), so the two patterns are two operators.  ragged: row r
    keeps r mod (nb + 1) blocks, row 0 none.  skipped: every third row's second block and the
    very last block of the value array have column -1, and one row has only such blocks.  The
    value and x tensors are exactly as long as the operator needs."""
    op = Op(LAT, bi, bd, dtype)
    if pattern == "ragged":
        op.keep(np.arange(op.vol) % (op.nb + 1))
        assert op.ii[0] == 0 and op.ii.max() == op.nb
    else:
        jj = op.jj.reshape(op.vol, op.nb, 6)
        jj[::3, 1, :] = -1
        jj[-1, op.nb - 1, :] = -1
        jj[-2, :, :] = -1
    assert op.vals.size == int(op.ii.sum()) * bi * bd
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = op.create(gpu)
    y, form = apply(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert form == FORM, form
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("lat", [(1, 3, 1, 5), (3, 2, 1, 3)])
@pytest.mark.parametrize("bi,bd,dtype,ncols", [(16, 16, C64, 12), (48, 48, C128, 17)])
def test_blocks_row_counts(gpu, lat, bi, bd, dtype, ncols):
    """15 and 18 block rows (the kernel takes one block row per workgroup: no partial workgroup)"""
    op = Op(lat, bi, bd, dtype)
    assert op.vol in (15, 18)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = op.create(gpu)
    y, form = apply(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert form == FORM, form
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd", [(48, 48), (20, 36)])
def test_blocks_adjoint(gpu, bi, bd):
    """A^H products (x with the image labels) land on the same kernel through the transposed
    operator; exact against the oracle's adjoint loop."""
    ncols, dtype = 12, C128
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = np.zeros(op.vol * bd * ncols, dtype)
    oracle_bsr_adjoint(TYPE_OF[op.dtype], op.dimd, 0, op.vol, bi, bd, op.ii, op.jj.reshape(-1),
                       op.vals, False, x, ncols, True, ref, ncols, True, op.vol * bd, ncols, 1.0)
    h = op.create(gpu)
    y, form = apply(gpu, op, h, x, y0, ncols, adjoint=True)
    h.destroy()
    assert form == FORM, form
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("key,value", [("bsr.blk_mfma", 0), ("bsr.variant", 1)])
def test_blocks_off_switch(gpu, key, value):
    import superbblas_amd as sb
    bi = bd = 48
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = op.create(gpu)
    y1, form1 = apply(gpu, op, h, x, y0, ncols)
    old = sb.tune_get(key)
    sb.tune_set(key, value)
    try:
        y0_, form0 = apply(gpu, op, h, x, y0, ncols)
    finally:
        sb.tune_set(key, old)
    h.destroy()
    assert (form1, form0) == (FORM, 0)
    assert np.array_equal(y1, ref) and np.array_equal(y0_, ref)


@pytest.mark.parametrize("bi,bd,dtype,ncols,by_default", [(16, 16, C128, 4, 0), (16, 16, C128, 12, FORM),
                                                         (24, 24, C128, 1, 0), (24, 24, C64, 4, FORM),
                                                         (32, 32, C128, 1, FORM)])
def test_blocks_column_bound(gpu, bi, bd, dtype, ncols, by_default):
    """The default dispatch keeps small blocks with few rhs columns on the generic kernel (where
    this kernel was measured no faster); "bsr.blk_mfma" 2 takes them anyway, with the same exact
    result."""
    import superbblas_amd as sb
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = op.create(gpu)
    y1, form1 = apply(gpu, op, h, x, y0, ncols)
    sb.tune_set("bsr.blk_mfma", 2)
    try:
        y2, form2 = apply(gpu, op, h, x, y0, ncols)
    finally:
        sb.tune_set("bsr.blk_mfma", 1)
    h.destroy()
    assert (form1, form2) == (by_default, FORM)
    assert np.array_equal(y1, ref) and np.array_equal(y2, ref)


@pytest.mark.parametrize("spin,color,ncols,forms", [(4, 3, 3, (7, 8)), (1, 3, 2, (1, 2, 3)),
                                                    (2, 3, 3, (0,))])
def test_blocks_floor(gpu, spin, color, ncols, forms):
    """12x12 and 3x3 operators keep their kernels and a 6x6 operator the generic one, with the new
    keys at their defaults"""
    import torch
    import superbblas_amd as sb
    from test_gpu_bsr import lattice_operator
    assert sb.tune_get("bsr.blk_mfma") == 1 and sb.tune_get("bsr.blk_min") == 16
    L = 4
    dim, ii, jj, vals, nb = lattice_operator(L, spin, color)
    b, vol = spin * color, L ** 4
    x = int_valued(vol * b * ncols, C128, 2)
    ref = np.zeros(vol * b * ncols, C128)
    oracle_bsr(TYPE_OF[np.dtype(C128)], dim, 0, vol, b, b, ii, jj, vals, False, x, ncols, True, ref,
               ncols, True, ncols, 1.0)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, spin, color]
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj).to(gpu)], [torch.from_numpy(vals).to(gpu)])
    dimx = [1, L, L, L, L, spin, color, ncols]
    ty = torch.zeros(vol * b * ncols, dtype=torch.complex128, device=gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                  dimx, "p", [ty])
    torch.cuda.synchronize()
    form = sb.tune_get("bsr.last_kernel")
    h.destroy()
    assert form in forms, form
    assert np.array_equal(ty.cpu().numpy(), ref)


def test_blocks_deterministic(gpu):
    bi = bd = 48
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype, values=random_valued)
    x = random_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    h = op.create(gpu)
    ya, fa = apply(gpu, op, h, x, y0, ncols)
    yb, fb = apply(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (fa, fb) == (FORM, FORM)
    assert np.array_equal(ya.view(np.uint8), yb.view(np.uint8))


@pytest.mark.parametrize("dtype,u", [(C64, 2.0 ** -24), (C128, 2.0 ** -53)])
def test_blocks_accuracy(gpu, dtype, u):
    """Random data in [-1, 1], 64x64 blocks, five per row, 12 columns, against the same product
    in numpy complex128 from the same rounded inputs.  Gate: the classical inner-product forward
    bound, ||y - y64||_2 / || |A| |x| ||_2 <= 2 (2 nnz bd + 4) u, which holds for any summation
    order (derived, not measured).  Measured on the MI355X (this kernel / the generic kernel):
    complex<float> 2.889e-08 / 2.869e-08, complex<double> 6.630e-17 / 6.641e-17, against the
    gates 7.677e-05 and 1.430e-13."""
    import superbblas_amd as sb
    bi = bd = 64
    ncols = 12
    op = Op(LAT, bi, bd, dtype, values=random_valued)
    x = random_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    cols = np.ravel_multi_index(tuple(op.sites[..., d] for d in range(4)), op.lat)  # [vol, nb]
    A = op.vals.reshape(op.vol, op.nb, bi, bd).astype(np.complex128)
    X = x.reshape(op.vol, bd, ncols).astype(np.complex128)[cols]                   # [vol, nb, bd, n]
    y64 = np.einsum("rjab,rjbn->ran", A, X).reshape(-1)
    scale = np.linalg.norm(np.einsum("rjab,rjbn->ran", np.abs(A), np.abs(X)))
    gate = 2 * (2 * op.nb * bd + 4) * u
    h = op.create(gpu)
    y1, f1 = apply(gpu, op, h, x, y0, ncols)
    sb.tune_set("bsr.blk_mfma", 0)
    try:
        yg, fg = apply(gpu, op, h, x, y0, ncols)
    finally:
        sb.tune_set("bsr.blk_mfma", 1)
    h.destroy()
    e1 = np.linalg.norm(y1.astype(np.complex128) - y64) / scale
    eg = np.linalg.norm(yg.astype(np.complex128) - y64) / scale
    msg = "%s: blk_mfma 1 err %.3e, blk_mfma 0 err %.3e, gate %.3e" % (np.dtype(dtype).name, e1, eg, gate)
    print(msg)
    assert (f1, fg) == (FORM, 0), (f1, fg)
    assert e1 <= gate and eg <= gate, msg


def test_blocks_values_beyond_2_31_bytes(gpu):
    """64x64 complex<double> blocks on a (4,5,5,37) lattice, nine per row: 3700 rows whose values
    end past 2^31 bytes; the first and the last 64 rows (the last ones lie past that offset)
    exact against the oracle on their slices of the operator and the whole x."""
    import torch
    import superbblas_amd as sb
    if torch.cuda.mem_get_info()[0] < 8e9:
        pytest.skip("less than 8 GB of device memory free")
    lat, b, nb, dtype = [4, 5, 5, 37], 64, 9, C128
    vol = int(np.prod(lat))
    dim = lat + list(split(b))
    jj = stencil_jj(lat).reshape(-1, 6)
    ii = np.full(vol, nb, np.int32)
    nv = vol * nb * b * b
    assert nv * 16 > 2 ** 31 and (vol - 64) * nb * b * b * 16 < 2 ** 31 < (vol - 32) * nb * b * b * 16
    tv = torch.empty(nv, dtype=torch.complex128, device=gpu)
    k = torch.arange(nv, dtype=torch.int64, device=gpu)
    tr = torch.view_as_real(tv)
    tr[:, 0] = ((k * 7 + 3) % 11 - 5).to(torch.float64)
    tr[:, 1] = ((k * 5 + 1) % 13 - 6).to(torch.float64)
    del k
    x = int_valued(vol * b, dtype, 2)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1] + list(split(b))
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj.reshape(-1)).to(gpu)], [tv])
    dimx = [1] + lat + list(split(b)) + [1]
    ty = torch.full((vol * b,), 7.0, dtype=torch.complex128, device=gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                  dimx, "p", [ty])
    torch.cuda.synchronize()
    form = sb.tune_get("bsr.last_kernel")
    y = ty.cpu().numpy()
    for r0 in (0, vol - 64):
        vs = tv[r0 * nb * b * b:(r0 + 64) * nb * b * b].cpu().numpy()
        ref = np.zeros(64 * b, dtype)
        oracle_bsr(TYPE_OF[np.dtype(dtype)], dim, 0, 64, b, b, ii[r0:r0 + 64],
                   np.ascontiguousarray(jj[r0 * nb:(r0 + 64) * nb]).reshape(-1), vs, False, x, 1, True,
                   ref, 1, True, 1, 1.0)
        assert np.array_equal(y[r0 * b:(r0 + 64) * b], ref), r0
    h.destroy()
    del tv
    assert form == FORM, form
