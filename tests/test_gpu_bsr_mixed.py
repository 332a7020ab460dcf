"""Mixed-precision bsr_krylov: an operator created in float / complex<float> applied to double /
complex<double> vectors (an extension of this library; the reference's bsr_krylov is one type
throughout).  The values are read in place in their own type and widened at the load, products
and sums are FP64: the result is the product of the up-converted operator with x.  Dense blocks
of 16 x 16 and more run bsr_blk_mfma_kernel's mixed form ("bsr.last_kernel" 16), everything else
the generic bsr_kernel's (0); "bsr.last_mixed" reads 1 after either.

Exact against the oracle's builtin BSR loop in the double type on vals.astype(double type) (the
conversion is exact) with integer-valued data: components are at most 6, a product component at
most 61 and a row sum at most 6 * 128 * 61 < 2^24, so every sum is exact in any order."""
import numpy as np
import pytest

from _common import TYPE_OF, int_valued, oracle_bsr, oracle_bsr_adjoint, random_valued
from test_gpu_bsr_blocks import Op, apply, layout, sentinel, split, stencil  # noqa: F401

pytestmark = pytest.mark.gpu

FORM = 16
LAT = (2, 2, 2, 2)
C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
WIDE = {np.dtype(C64): np.dtype(C128), np.dtype(F32): np.dtype(F64)}


def wide(op):
    return WIDE[op.dtype]


def create(op, gpu, im_fast=False, values=None):
    """the operator in its own (single-precision) type; values: a device tensor to use as it is"""
    import torch
    import superbblas_amd as sb
    pi, pd = [([0] * 6, op.dimi)], [([0] * 6, op.dimd)]
    tv = torch.from_numpy(op.vals).to(gpu) if values is None else values
    return sb.create_bsr(pi, op.dimi, pd, op.dimd, [1, 1, 1, 1] + list(split(op.bi)),
                         [1, 1, 1, 1] + list(split(op.bd)), im_fast,
                         [torch.from_numpy(op.ii).to(gpu)],
                         [torch.from_numpy(op.jj.reshape(-1)).to(gpu)], [tv])


def reference(op, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, im_fast=False):
    """the oracle's loop in x's (double) type on the up-converted values"""
    assert x.dtype == wide(op) and y0.dtype == wide(op)
    y = (beta * y0).astype(x.dtype)
    oracle_bsr(TYPE_OF[x.dtype], op.dimd, 0, op.vol, op.bi, op.bd, op.ii, op.jj.reshape(-1),
               op.vals.astype(x.dtype), im_fast, x, ncols if xrow else op.vol * op.bd, xrow, y,
               ncols if yrow else op.vol * op.bi, yrow, ncols, alpha, add=True)
    return y


def run(gpu, op, h, x, y0, ncols, **kw):
    """apply of test_gpu_bsr_blocks (the types come from x and y0) and the two read-backs"""
    import superbblas_amd as sb
    y, form = apply(gpu, op, h, x, y0, ncols, **kw)
    return y, form, sb.tune_get("bsr.last_mixed")


class tuned:
    """tune keys set for a block and restored after it"""

    def __init__(self, **keys):
        self.keys = {"bsr." + k: v for k, v in keys.items()}

    def __enter__(self):
        import superbblas_amd as sb
        self.old = {k: sb.tune_get(k) for k in self.keys}
        for k, v in self.keys.items():
            sb.tune_set(k, v)

    def __exit__(self, *exc):
        import superbblas_amd as sb
        for k, v in self.old.items():
            sb.tune_set(k, v)


# (block) x (pair) x (columns) x (x layout) x (y layout) x (block_im_fast) x (blk_mfma 2: the
# default dispatch leaves small blocks with few rhs columns to the generic form).  Every block
# with either pair and every column count with either pair; each pair has a block row that is
# no 16-byte multiple in the operator's type ((20,21) for both, (18,22) for float), a bd that is
# no multiple of 4 VA (8 for complex<float>: 36, 21, 22; 16 for float: 24, 36, 21, 22), partial
# column tiles (1, 3, 12, 17, 40) and blocks of one (16 rows), two (18-32 rows) and more strips.
EXACT = [
    (16, 16, C64, 1, True, True, False, 2), (16, 16, C64, 16, False, True, True, 1),
    (24, 24, C64, 3, True, False, False, 2), (24, 24, C64, 12, False, False, True, 1),
    (48, 48, C64, 12, True, True, False, 1), (48, 48, C64, 17, False, True, True, 1),
    (64, 64, C64, 40, True, False, False, 1), (64, 64, C64, 1, True, True, True, 1),
    (20, 36, C64, 17, False, False, False, 1), (20, 36, C64, 40, True, True, True, 1),
    (20, 21, C64, 3, True, True, False, 2), (20, 21, C64, 16, True, False, True, 1),
    (18, 22, C64, 12, False, True, False, 1), (18, 22, C64, 1, True, False, True, 2),
    (32, 16, C64, 40, True, True, True, 1), (32, 16, C64, 3, False, False, False, 2),
    (16, 80, C64, 17, True, False, False, 1), (16, 80, C64, 16, False, True, True, 1),
    (128, 128, C64, 12, True, True, False, 1), (128, 128, C64, 3, False, False, True, 1),
    (16, 16, F32, 12, True, False, False, 1), (16, 16, F32, 3, False, False, True, 2),
    (24, 24, F32, 17, True, True, False, 1), (24, 24, F32, 1, False, True, True, 2),
    (48, 48, F32, 40, True, True, False, 1), (48, 48, F32, 3, False, False, True, 1),
    (64, 64, F32, 16, False, True, False, 1), (64, 64, F32, 12, True, False, True, 1),
    (20, 36, F32, 12, True, True, True, 1), (20, 36, F32, 1, True, False, False, 2),
    (20, 21, F32, 17, False, True, False, 1), (20, 21, F32, 40, True, True, True, 1),
    (18, 22, F32, 40, True, False, True, 1), (18, 22, F32, 3, True, True, False, 2),
    (32, 16, F32, 16, False, False, False, 1), (32, 16, F32, 1, True, True, True, 2),
    (16, 80, F32, 40, False, True, True, 1), (16, 80, F32, 12, True, True, False, 1),
    (128, 128, F32, 17, True, False, False, 1), (128, 128, F32, 1, False, True, True, 1),
]


@pytest.mark.parametrize("bi,bd,dtype,ncols,xrow,yrow,imf,blk_mfma", EXACT)
def test_mixed_exact(gpu, bi, bd, dtype, ncols, xrow, yrow, imf, blk_mfma):
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = sentinel(op.vol * bi * ncols, wide(op))
    ref = reference(op, x, y0, ncols, xrow, yrow, im_fast=imf)
    h = create(op, gpu, imf)
    with tuned(blk_mfma=blk_mfma):
        y, form, mixed = run(gpu, op, h, x, y0, ncols, xrow=xrow, yrow=yrow)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert y.dtype == wide(op) and np.array_equal(y, ref)


def test_mixed_unaligned_values(gpu):
    """the value tensor starts one element into its buffer: 8-byte aligned only, so every
    fragment goes element by element; the buffer ends with the operator's last value"""
    import torch
    bi = bd = 48
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype)
    buf = torch.empty(op.vals.size + 1, dtype=torch.complex64, device=gpu)
    tv = buf[1:]
    tv.copy_(torch.from_numpy(op.vals))
    assert tv.data_ptr() % 16 == 8
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = sentinel(op.vol * bi * ncols, wide(op))
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu, values=tv)
    y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd,dtype", [(48, 48, C64), (20, 36, F32)])
@pytest.mark.parametrize("alpha,beta", [(2 - 1j, 1.0), (-1.0, 0.0)])
def test_mixed_alpha_beta(gpu, bi, bd, dtype, alpha, beta):
    ncols = 5
    if np.dtype(dtype).kind != "c":
        alpha = alpha.real
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = int_valued(op.vol * bi * ncols, wide(op), 3)
    ref = reference(op, x, y0, ncols, alpha=alpha, beta=beta)
    h = create(op, gpu)
    y, form, mixed = run(gpu, op, h, x, y0, ncols, alpha=alpha, beta=beta)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pattern", ["ragged", "skipped"])
@pytest.mark.parametrize("bi,bd,dtype,ncols,blk_mfma", [(48, 48, C64, 13, 1), (48, 48, C64, 16, 1),
                                                        (20, 21, C64, 5, 2), (20, 21, F32, 5, 2)])
def test_mixed_ragged_and_skipped(gpu, bi, bd, dtype, ncols, blk_mfma, pattern):
    """The two patterns of test_gpu_bsr_blocks.test_blocks_ragged_and_skipped (ragged: row r keeps
    r mod (nb + 1) blocks; skipped: column -1 on every third row's second block, on the very last
    block of the value array and on a whole row), the value and x tensors exactly as long as the
    operator needs.  (20,21): rows that are no 16-byte multiple, every fragment by elements (a
    small block with few columns: "bsr.blk_mfma" 2)."""
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
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = sentinel(op.vol * bi * ncols, wide(op))
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    with tuned(blk_mfma=blk_mfma):
        y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("lat", [(1, 3, 1, 5), (3, 2, 1, 3)])
@pytest.mark.parametrize("bi,bd,dtype,ncols", [(16, 16, C64, 12), (48, 48, F32, 17)])
def test_mixed_row_counts(gpu, lat, bi, bd, dtype, ncols):
    """15 and 18 block rows (one block row per workgroup: no partial workgroup)"""
    op = Op(lat, bi, bd, dtype)
    assert op.vol in (15, 18)
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = sentinel(op.vol * bi * ncols, wide(op))
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd", [(48, 48), (20, 36)])
def test_mixed_adjoint(gpu, bi, bd):
    """x with the image labels: A^H x through the transposed operator, which stays complex<float>"""
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, C128, 2)
    y0 = sentinel(op.vol * bd * ncols, C128)
    ref = np.zeros(op.vol * bd * ncols, C128)
    oracle_bsr_adjoint(TYPE_OF[np.dtype(C128)], op.dimd, 0, op.vol, bi, bd, op.ii, op.jj.reshape(-1),
                       op.vals.astype(C128), False, x, ncols, True, ref, ncols, True, op.vol * bd,
                       ncols, 1.0)
    h = create(op, gpu)
    y, form, mixed = run(gpu, op, h, x, y0, ncols, adjoint=True)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


def test_mixed_x_through_a_temporary(gpu):
    """x ordered pXYnZTSC -- neither row nor column major -- is copied to a temporary, which is
    complex<double> like x"""
    import torch
    import superbblas_amd as sb
    bi = bd = 24
    ncols = 12
    op = Op(LAT, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    ref = reference(op, x, y0, ncols)
    s, c = split(bd)
    xdev = np.ascontiguousarray(x.reshape(*LAT, s, c, ncols).transpose(0, 1, 6, 2, 3, 4, 5)).reshape(-1)
    dimx = [1, LAT[0], LAT[1], ncols, LAT[2], LAT[3], s, c]
    oy, dimy = layout(LAT, bi, ncols, True, False)
    h = create(op, gpu)
    ty = torch.from_numpy(y0.copy()).to(gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYnZTSC", [0] * 8, dimx, dimx,
                  [torch.from_numpy(xdev).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                  "p", [ty])
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(ty.cpu().numpy(), ref)


def test_mixed_two_components_halo(gpu):
    """one process, two components: the image of a (4,2,2,2) lattice split in two along x, each
    component's domain its image plus a one-site halo in every direction (here the whole
    lattice), x and y split like the image: x reaches the domain partition through the halo
    exchange, in complex<double>"""
    import torch
    import superbblas_amd as sb
    lat, bi, bd, ncols = (4, 2, 2, 2), 24, 24, 12
    op = Op(lat, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    ref = reference(op, x, y0, ncols)
    pi = [([2 * c, 0, 0, 0, 0, 0], [2, 2, 2, 2] + list(split(bi))) for c in range(2)]
    pd = [([0] * 6, op.dimd) for c in range(2)]
    half = op.vol // 2  # rows 0 .. half - 1 are the sites with x < 2 (x is the slowest coordinate)
    rows = op.vals.size // op.vol
    cii = [torch.from_numpy(op.ii[c * half:(c + 1) * half].copy()).to(gpu) for c in range(2)]
    cjj = [torch.from_numpy(op.jj[c * half * op.nb:(c + 1) * half * op.nb].reshape(-1).copy()).to(gpu)
           for c in range(2)]
    cv = [torch.from_numpy(op.vals[c * half * rows:(c + 1) * half * rows].copy()).to(gpu) for c in range(2)]
    h = sb.create_bsr(pi, op.dimi, pd, op.dimd, [1, 1, 1, 1] + list(split(bi)),
                      [1, 1, 1, 1] + list(split(bd)), False, cii, cjj, cv)
    dimx = [1] + list(lat) + list(split(bd)) + [ncols]
    hx = [1, 2] + dimx[2:]
    px = [([0, 2 * c, 0, 0, 0, 0, 0, 0], hx) for c in range(2)]
    n2 = x.size // 2
    vx = [torch.from_numpy(x[c * n2:(c + 1) * n2].copy()).to(gpu) for c in range(2)]
    vy = [torch.from_numpy(y0[c * n2:(c + 1) * n2].copy()).to(gpu) for c in range(2)]
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", px, "pXYZTSCn", [0] * 8, dimx, dimx, vx, 0.0, px,
                  "pxyztscn", [0] * 8, dimx, dimx, "p", vy)
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(np.concatenate([v.cpu().numpy() for v in vy]), ref)


def test_mixed_powers(gpu):
    """y[p] = A^(p+1) x for p = 0, 1 on a square 16x16 operator: the first power's image pieces
    become the second one's x, all in complex<double>.  A component of A x is at most
    5 * 16 * 2 * 36 = 5760 in size and one of A^2 x at most 5 * 16 * 2 * 6 * 5760 < 2^23: exact."""
    import torch
    import superbblas_amd as sb
    b, ncols = 16, 12
    op = Op(LAT, b, b, C64)
    x = int_valued(op.vol * b * ncols, C128, 2)
    zero = np.zeros(op.vol * b * ncols, C128)
    y1 = reference(op, x, zero, ncols)
    y2 = reference(op, y1, zero, ncols)
    ox, dimx = layout(LAT, b, ncols, True, True)
    oy, _ = layout(LAT, b, ncols, True, False)
    dimy = [2] + dimx[1:]
    h = create(op, gpu)
    ty = torch.from_numpy(sentinel(2 * op.vol * b * ncols, C128)).to(gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                  "p", [ty])
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(ty.cpu().numpy(), np.concatenate([y1, y2]))


@pytest.mark.parametrize("key,value", [("mixed", 0), ("blk_mfma", 0), ("variant", 1)])
def test_mixed_switches(gpu, key, value):
    """each switch sends the mixed product to the generic mixed form: the same exact result"""
    bi = bd = 48
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, wide(op), 2)
    y0 = sentinel(op.vol * bi * ncols, wide(op))
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y1, form1, mixed1 = run(gpu, op, h, x, y0, ncols)
    with tuned(**{key: value}):
        y0_, form0, mixed0 = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form1, mixed1, form0, mixed0) == (FORM, 1, 0, 1)
    assert np.array_equal(y1, ref) and np.array_equal(y0_, ref)


@pytest.mark.parametrize("bi,bd,ncols,by_default", [(16, 16, 1, 0), (16, 16, 4, FORM), (24, 24, 3, 0),
                                                    (32, 32, 1, FORM)])
def test_mixed_column_bound(gpu, bi, bd, ncols, by_default):
    """The default dispatch keeps blocks of fewer than 1024 elements with fewer than 4 rhs columns
    on the generic mixed form (where the matrix-core form was measured no faster);
    "bsr.blk_mfma" 2 takes them anyway, with the same exact result."""
    op = Op(LAT, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y1, form1, _ = run(gpu, op, h, x, y0, ncols)
    with tuned(blk_mfma=2):
        y2, form2, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form1, form2) == (by_default, FORM)
    assert np.array_equal(y1, ref) and np.array_equal(y2, ref)


@pytest.mark.parametrize("spin,color", [(1, 3), (2, 3), (4, 3)])
def test_mixed_small_blocks(gpu, spin, color):
    """3x3, 6x6 and 12x12 operators in complex<float> with complex<double> vectors: the generic
    mixed form (their specialised kernels are one type throughout)"""
    import torch
    import superbblas_amd as sb
    from test_gpu_bsr import lattice_operator
    L, ncols = 4, 3
    dim, ii, jj, vals, nb = lattice_operator(L, spin, color, C64)
    b, vol = spin * color, L ** 4
    x = int_valued(vol * b * ncols, C128, 2)
    ref = np.zeros(vol * b * ncols, C128)
    oracle_bsr(TYPE_OF[np.dtype(C128)], dim, 0, vol, b, b, ii, jj, vals.astype(C128), False, x, ncols,
               True, ref, ncols, True, ncols, 1.0)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, spin, color]
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj).to(gpu)], [torch.from_numpy(vals).to(gpu)])
    dimx = [1, L, L, L, L, spin, color, ncols]
    ty = torch.full((vol * b * ncols,), 7.0, dtype=torch.complex128, device=gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                  dimx, "p", [ty])
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (0, 1), (form, mixed)
    assert np.array_equal(ty.cpu().numpy(), ref)


@pytest.mark.parametrize("mixed_key", [1, 0])
def test_mixed_values_read_in_place(gpu, mixed_key):
    """the operator reads the caller's value tensor at every product: scaled by 2 on the device
    after the first product, the second product is twice the first (no converted copy is kept)"""
    import torch
    bi = bd = 48
    ncols = 12
    op = Op(LAT, bi, bd, C64)
    tv = torch.from_numpy(op.vals).to(gpu)
    x = int_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu, values=tv)
    with tuned(mixed=mixed_key):
        y1, form1, _ = run(gpu, op, h, x, y0, ncols)
        tv.mul_(2)
        torch.cuda.synchronize()
        y2, form2, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert form1 == form2 == (FORM if mixed_key else 0)
    assert np.array_equal(y1, ref) and np.array_equal(y2, 2 * ref)


def test_mixed_accuracy(gpu):
    """Random data in [-1, 1], 64x64 complex<float> blocks, five per row, 12 columns of
    complex<double> x, against numpy complex128 from the up-converted values.  Gate: the
    inner-product forward bound in FP64 for any summation order, as test_blocks_accuracy derives
    it for complex<double>: ||y - y64||_2 / || |A| |x| ||_2 <= 2 (2 nb bd + 4) 2^-53 = 1.43e-13.
    Rounding x, a partial sum or y to float would leave an error near 2^-24 = 6e-8.  Measured on
    the MI355X: 6.646e-17 (matrix-core form) and 6.608e-17 (generic mixed form)."""
    bi = bd = 64
    ncols = 12
    op = Op(LAT, bi, bd, C64, values=random_valued)
    x = random_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    cols = np.ravel_multi_index(tuple(op.sites[..., d] for d in range(4)), op.lat)  # [vol, nb]
    A = op.vals.reshape(op.vol, op.nb, bi, bd).astype(np.complex128)
    X = x.reshape(op.vol, bd, ncols)[cols]                                          # [vol, nb, bd, n]
    y64 = np.einsum("rjab,rjbn->ran", A, X).reshape(-1)
    scale = np.linalg.norm(np.einsum("rjab,rjbn->ran", np.abs(A), np.abs(X)))
    gate = 2 * (2 * op.nb * bd + 4) * 2.0 ** -53
    h = create(op, gpu)
    y1, f1, m1 = run(gpu, op, h, x, y0, ncols)
    with tuned(mixed=0):
        yg, fg, mg = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    e1 = np.linalg.norm(y1 - y64) / scale
    eg = np.linalg.norm(yg - y64) / scale
    msg = "mixed 1 err %.3e, mixed 0 err %.3e, gate %.3e" % (e1, eg, gate)
    print(msg)
    assert (f1, m1, fg, mg) == (FORM, 1, 0, 1), (f1, m1, fg, mg)
    assert e1 <= gate and eg <= gate, msg


def test_mixed_deterministic(gpu):
    bi = bd = 64
    ncols = 12
    op = Op(LAT, bi, bd, C64, values=random_valued)
    x = random_valued(op.vol * bd * ncols, C128, 2)
    y0 = sentinel(op.vol * bi * ncols, C128)
    h = create(op, gpu)
    ya, fa, _ = run(gpu, op, h, x, y0, ncols)
    yb, fb, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (fa, fb) == (FORM, FORM)
    assert np.array_equal(ya.view(np.uint8), yb.view(np.uint8))


@pytest.mark.parametrize("vt,xt,yt", [(C128, C64, C64), (C64, F64, F64), (F32, C128, C128),
                                      (C64, C128, C64)])
def test_mixed_refused_pairs(gpu, vt, xt, yt):
    """every pair but float -> double and complex<float> -> complex<double> keeps raising, and y
    keeps its sentinel"""
    import torch
    import superbblas_amd as sb
    bi = bd = 16
    ncols = 12
    op = Op(LAT, bi, bd, vt)
    h = create(op, gpu)
    ox, dimx = layout(LAT, bd, ncols, True, True)
    oy, dimy = layout(LAT, bi, ncols, True, False)
    tx = torch.from_numpy(int_valued(op.vol * bd * ncols, xt, 2)).to(gpu)
    ty = torch.from_numpy(sentinel(op.vol * bi * ncols, yt)).to(gpu)
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx, [tx],
                          0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy, "p", [ty])
        torch.cuda.synchronize()
    finally:
        h.destroy()
    assert np.array_equal(ty.cpu().numpy(), sentinel(op.vol * bi * ncols, yt))


def test_mixed_refused_kronecker(gpu):
    """an operator of create_kron_bsr in complex<float> with complex<double> vectors"""
    import torch
    import superbblas_amd as sb
    from test_gpu_kron_bsr import kron_lattice
    L, spin, color, ncols = 4, 4, 3, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    h = sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False,
                           [torch.from_numpy(ii).to(gpu)], [torch.from_numpy(jj).to(gpu)],
                           [torch.from_numpy(vals.astype(C64)).to(gpu)],
                           [torch.from_numpy(kron.astype(C64)).to(gpu)])
    n = L ** 4 * color * ncols * spin
    dimx = [1, L, L, L, L, color, ncols, spin]
    tx = torch.from_numpy(int_valued(n, C128, 2)).to(gpu)
    ty = torch.from_numpy(sentinel(n, C128)).to(gpu)
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTCnS", [0] * 8, dimx,
                          dimx, [tx], 0.0, [([0] * 8, dimx)], "pxyztcns", [0] * 8, dimx, dimx, "p", [ty])
        torch.cuda.synchronize()
    finally:
        h.destroy()
    assert np.array_equal(ty.cpu().numpy(), sentinel(n, C128))
