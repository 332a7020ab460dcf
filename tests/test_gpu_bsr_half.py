"""Half-precision bsr_krylov: an operator created in float16 / complex32 (IEEE binary16; re, im)
applied to float32 / complex64 vectors (an extension of this library).  The values are read in
place in their own type and widened at the load (exact, subnormals included); products, sums,
alpha, beta and y are FP32: the result is the product of the widened operator with x.  Dense
blocks of 16 x 16 and more run bsr_blk_mfma_kernel's mixed form ("bsr.last_kernel" 16), everything
else the generic bsr_kernel's (0, or 18 for the in-place adjoint); "bsr.last_mixed" reads 1.

The operators are built in complex64 / float32 integer data and converted on the host.  Exact
against the oracle's builtin BSR loop in the float type on the values widened to float:
components are at most 6 (exact in binary16), a product component at most 61 and a row sum at
most 6 * 128 * 61 < 2^24, so every sum is exact in float in any order (the argument of
test_gpu_bsr_mixed.py and test_gpu_bsr_blocks.py)."""
import numpy as np
import pytest

from _common import TYPE_OF, int_valued, oracle_bsr, oracle_bsr_adjoint, random_valued
from test_gpu_bsr_blocks import Op, apply, layout, sentinel, split

pytestmark = pytest.mark.gpu

FORM = 16
LAT = (2, 2, 2, 2)
C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64


def to_half(vals):
    """complex64 / float32 values rounded to binary16 on the host: a float16 array, (re, im)
    interleaved for complex values"""
    v = np.ascontiguousarray(vals)
    return (v.view(np.float32) if v.dtype.kind == "c" else v).astype(np.float16)


def widened(h16, cplx):
    """the binary16 values as float32 / complex64 (exact)"""
    f = np.ascontiguousarray(h16).astype(np.float32)
    return f.view(np.complex64) if cplx else f


def device_values(h16, cplx, gpu, lead=0):
    """(the float16 / complex32 value tensor, its float16 view); lead: the tensor starts that many
    elements into its buffer, which ends with the last value"""
    import torch
    per = 2 if cplx else 1
    buf = torch.empty(h16.size + lead * per, dtype=torch.float16, device=gpu)
    t16 = buf[lead * per:]
    t16.copy_(torch.from_numpy(np.ascontiguousarray(h16)))
    return (torch.view_as_complex(t16.view(-1, 2)) if cplx else t16), t16


def create(op, gpu, im_fast=False, values=None):
    """the operator in half precision, op.vals converted (exactly: asserted); values: a device
    tensor to use as it is"""
    import torch
    import superbblas_amd as sb
    cplx = op.dtype.kind == "c"
    if values is None:
        h16 = to_half(op.vals)
        assert np.array_equal(widened(h16, cplx), op.vals)
    tv = device_values(h16, cplx, gpu)[0] if values is None else values
    assert tv.dtype == (torch.complex32 if cplx else torch.float16)
    pi, pd = [([0] * 6, op.dimi)], [([0] * 6, op.dimd)]
    return sb.create_bsr(pi, op.dimi, pd, op.dimd, [1, 1, 1, 1] + list(split(op.bi)),
                         [1, 1, 1, 1] + list(split(op.bd)), im_fast,
                         [torch.from_numpy(op.ii).to(gpu)],
                         [torch.from_numpy(op.jj.reshape(-1)).to(gpu)], [tv])


def reference(op, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, im_fast=False, vals=None):
    """the oracle's loop in the float type on the values widened to float"""
    vals = op.vals if vals is None else vals
    assert x.dtype == op.dtype and y0.dtype == op.dtype and vals.dtype == op.dtype
    y = (beta * y0).astype(x.dtype)
    oracle_bsr(TYPE_OF[x.dtype], op.dimd, 0, op.vol, op.bi, op.bd, op.ii, op.jj.reshape(-1),
               vals, im_fast, x, ncols if xrow else op.vol * op.bd, xrow, y,
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


# (block) x (pair: the vectors' type) x (columns) x (x layout) x (y layout) x (block_im_fast) x
# (blk_mfma 2: the default dispatch leaves small blocks with few rhs columns to the generic form).
# Every block and every column count with either pair.  A k-step is 4 VA = 16 k (complex32) or 32 k
# (float16): 16x16 is one strip whose real k-step is half padding; 64x64 has 4 / 2 k-steps; 16x80
# 5 / 3 k-steps split over four k-parts; 128x128 is eight strips and NT 1.  Rows that are no
# 16-byte multiple (bd % 4 != 0 complex, bd % 8 != 0 real): (20,21) and (18,22) for both, (20,36)
# for real; bd no multiple of VA: 21, 22 (and 36 for real); partial column tiles 1, 3, 12, 17, 40.
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
def test_half_exact(gpu, bi, bd, dtype, ncols, xrow, yrow, imf, blk_mfma):
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols, xrow, yrow, im_fast=imf)
    h = create(op, gpu, imf)
    with tuned(blk_mfma=blk_mfma):
        y, form, mixed = run(gpu, op, h, x, y0, ncols, xrow=xrow, yrow=yrow)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert y.dtype == op.dtype and np.array_equal(y, ref)


@pytest.mark.parametrize("dtype,align", [(C64, 4), (F32, 2)])
def test_half_unaligned_values(gpu, dtype, align):
    """the value tensor starts one element into its buffer: 4-byte aligned only (complex32) or
    2-byte aligned only (float16), so every fragment goes element by element; the buffer ends
    with the operator's last value"""
    bi = bd = 48
    ncols = 12
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    tv, _ = device_values(to_half(op.vals), op.dtype.kind == "c", gpu, lead=1)
    assert tv.data_ptr() % 16 == align and tv.numel() == op.vals.size
    h = create(op, gpu, values=tv)
    y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pattern", ["ragged", "skipped"])
@pytest.mark.parametrize("bi,bd,dtype,ncols,blk_mfma", [(48, 48, C64, 13, 1), (48, 48, C64, 16, 1),
                                                        (20, 21, C64, 5, 2), (20, 21, F32, 5, 2)])
def test_half_ragged_and_skipped(gpu, bi, bd, dtype, ncols, blk_mfma, pattern):
    """The two patterns of test_gpu_bsr_mixed.test_mixed_ragged_and_skipped (ragged: row r keeps
    r mod (nb + 1) blocks; skipped: column -1 on every third row's second block, on the very last
    block of the value array and on a whole row), the value and x tensors exactly as long as the
    operator needs.  (20,21): rows that are no 16-byte multiple, every fragment by elements."""
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
    h = create(op, gpu)
    with tuned(blk_mfma=blk_mfma):
        y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("lat", [(1, 3, 1, 5), (3, 2, 1, 3)])
@pytest.mark.parametrize("bi,bd,dtype,ncols", [(16, 16, C64, 12), (48, 48, F32, 17)])
def test_half_row_counts(gpu, lat, bi, bd, dtype, ncols):
    """15 and 18 block rows (one block row per workgroup: no partial workgroup)"""
    op = Op(lat, bi, bd, dtype)
    assert op.vol in (15, 18)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


# binary16 bit patterns: the largest finite value and its negative, the smallest normal 2^-14, the
# smallest subnormal 2^-24, subnormals with several mantissa bits (0x02ab = 683 * 2^-24), +-0, and
# ordinary values
SPECIAL_BITS = np.array([0x7bff, 0xfbff, 0x0400, 0x0001, 0x02ab, 0x82ab, 0x0000, 0x8000, 0x03ff,
                         0x8001, 0x3c00, 0xc500, 0x3555], np.uint16)


@pytest.mark.parametrize("dtype", [C64, F32])
@pytest.mark.parametrize("matrix_cores", [True, False])
def test_half_exact_widening(gpu, dtype, matrix_cores):
    """x holds the 16 unit vectors on site 0 and zeros elsewhere, 16 columns: a row's only block
    on site 0 (the stencil's sites of a row are distinct) appears in y widened, every other term
    of every sum is a zero -- no rounding anywhere.  The values cycle through 65504, -65504,
    2^-14, 2^-24, subnormals with several mantissa bits and +-0: a flushed subnormal or a
    saturated maximum shows as a wrong element."""
    b = ncols = 16
    op = Op(LAT, b, b, dtype)
    cplx = op.dtype.kind == "c"
    n16 = op.vals.size * (2 if cplx else 1)
    h16 = SPECIAL_BITS[(np.arange(n16) * 5 + np.arange(n16) // 7) % SPECIAL_BITS.size].view(np.float16)
    vals = widened(h16, cplx)
    assert np.all(np.isfinite(vals.view(np.float32)))
    assert np.float32(2.0 ** -24) in vals.view(np.float32) and np.float32(65504) in vals.view(np.float32)
    x = np.zeros((op.vol * b, ncols), dtype)
    x[np.arange(b), np.arange(b)] = 1
    x = x.reshape(-1)
    y0 = sentinel(op.vol * b * ncols, dtype)
    ref = reference(op, x, y0, ncols, vals=vals)
    # the reference is itself a copy of blocks: row 0's first block is the site's own
    assert np.array_equal(ref.reshape(op.vol, b, ncols)[0], vals.reshape(op.vol, op.nb, b, b)[0, 0])
    tv, _ = device_values(h16, cplx, gpu)
    h = create(op, gpu, values=tv)
    with tuned(mixed=1 if matrix_cores else 0):
        y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM if matrix_cores else 0, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd,dtype", [(48, 48, C64), (20, 36, F32)])
@pytest.mark.parametrize("alpha,beta", [(2 - 1j, 1.0), (-1.0, 0.0)])
def test_half_alpha_beta(gpu, bi, bd, dtype, alpha, beta):
    """(20x36 with 5 columns is below the default column bound: "bsr.blk_mfma" 2)"""
    ncols = 5
    if np.dtype(dtype).kind != "c":
        alpha = alpha.real
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = int_valued(op.vol * bi * ncols, dtype, 3)
    ref = reference(op, x, y0, ncols, alpha=alpha, beta=beta)
    h = create(op, gpu)
    with tuned(blk_mfma=2):
        y, form, mixed = run(gpu, op, h, x, y0, ncols, alpha=alpha, beta=beta)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


def adjoint_reference(op, x, ncols):
    ref = np.zeros(op.vol * op.bd * ncols, op.dtype)
    oracle_bsr_adjoint(TYPE_OF[op.dtype], op.dimd, 0, op.vol, op.bi, op.bd, op.ii, op.jj.reshape(-1),
                       op.vals, False, x, ncols, True, ref, ncols, True, op.vol * op.bd, ncols, 1.0)
    return ref


@pytest.mark.parametrize("bi,bd,dtype,per_element", [(48, 48, C64, 4), (20, 36, C64, 4), (48, 48, F32, 2)])
def test_half_adjoint_copy(gpu, bi, bd, dtype, per_element):
    """x with the image labels, "bsr.adj_inplace" 0: A^H x through the conjugated, regrouped copy,
    which stays in the operator's type -- "bsr.adj_copy_bytes" grows by 4 (complex32) or 2
    (float16) bytes per element -- on the matrix-core form"""
    import superbblas_amd as sb
    ncols = 12
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, ncols)
    h = create(op, gpu)
    before = sb.tune_get("bsr.adj_copy_bytes")
    with tuned(adj_inplace=0):
        y, form, mixed = run(gpu, op, h, x, y0, ncols, adjoint=True)
    held = sb.tune_get("bsr.adj_copy_bytes") - before
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert held == per_element * op.vals.size, (held, op.vals.size)
    assert sb.tune_get("bsr.adj_copy_bytes") == before
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd,dtype", [(48, 48, C64), (20, 36, C64), (48, 48, F32)])
def test_half_adjoint_inplace(gpu, bi, bd, dtype):
    """"bsr.adj_inplace" 1: A^H from A's own half-precision values through the generic in-place
    form (18), no copy"""
    import superbblas_amd as sb
    ncols = 12
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, ncols)
    h = create(op, gpu)
    before = sb.tune_get("bsr.adj_copy_bytes")
    with tuned(adj_inplace=1):
        y, form, mixed = run(gpu, op, h, x, y0, ncols, adjoint=True)
    held = sb.tune_get("bsr.adj_copy_bytes") - before
    h.destroy()
    assert (form, mixed, held) == (18, 1, 0), (form, mixed, held)
    assert np.array_equal(y, ref)


def test_half_x_through_a_temporary(gpu):
    """x ordered pXYnZTSC -- neither row nor column major -- is copied to a temporary, which is
    complex<float> like x"""
    import torch
    import superbblas_amd as sb
    bi = bd = 24
    ncols = 12
    op = Op(LAT, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
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


@pytest.mark.parametrize("dtype", [C64, F32])
def test_half_host_component(gpu, dtype):
    """ii, jj and the values in host memory (a CPU-context component): the half-precision values
    are mirrored to the device byte for byte at create_bsr, 4 / 2 bytes per element"""
    import torch
    import superbblas_amd as sb
    bi, bd, ncols = 20, 24, 12
    op = Op(LAT, bi, bd, dtype)
    cplx = op.dtype.kind == "c"
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    t16 = torch.from_numpy(to_half(op.vals))
    tv = torch.view_as_complex(t16.view(-1, 2)) if cplx else t16
    assert not tv.is_cuda and tv.numel() == op.vals.size
    pi, pd = [([0] * 6, op.dimi)], [([0] * 6, op.dimd)]
    h = sb.create_bsr(pi, op.dimi, pd, op.dimd, [1, 1, 1, 1] + list(split(bi)),
                      [1, 1, 1, 1] + list(split(bd)), False, [torch.from_numpy(op.ii)],
                      [torch.from_numpy(op.jj.reshape(-1))], [tv])
    y, form, mixed = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("level", [1, 2])
def test_half_debug_levels(gpu, level):
    """SB_DEBUG 1 / 2 ("debug.level"): the argument hash and the mock-index copy check run with a
    half-precision operator, x through a temporary (a copy in complex<float>)"""
    import torch
    import superbblas_amd as sb
    bi = bd = 24
    ncols = 12
    op = Op(LAT, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    ref = reference(op, x, y0, ncols)
    s, c = split(bd)
    xdev = np.ascontiguousarray(x.reshape(*LAT, s, c, ncols).transpose(0, 1, 6, 2, 3, 4, 5)).reshape(-1)
    dimx = [1, LAT[0], LAT[1], ncols, LAT[2], LAT[3], s, c]
    oy, dimy = layout(LAT, bi, ncols, True, False)
    h = create(op, gpu)
    ty = torch.from_numpy(y0.copy()).to(gpu)
    old = sb.tune_get("debug.level")
    sb.tune_set("debug.level", level)
    try:
        sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYnZTSC", [0] * 8, dimx, dimx,
                      [torch.from_numpy(xdev).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy,
                      dimy, "p", [ty])
        torch.cuda.synchronize()
    finally:
        sb.tune_set("debug.level", old)
        h.destroy()
    assert np.array_equal(ty.cpu().numpy(), ref)


def test_half_two_components_halo(gpu):
    """one process, two components: the image of a (4,2,2,2) lattice split in two along x, each
    component's domain the whole lattice, x and y split like the image: x reaches the domain
    partition through the halo exchange, in complex<float>"""
    import torch
    import superbblas_amd as sb
    lat, bi, bd, ncols = (4, 2, 2, 2), 24, 24, 12
    op = Op(lat, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    ref = reference(op, x, y0, ncols)
    pi = [([2 * c, 0, 0, 0, 0, 0], [2, 2, 2, 2] + list(split(bi))) for c in range(2)]
    pd = [([0] * 6, op.dimd) for c in range(2)]
    half = op.vol // 2  # rows 0 .. half - 1 are the sites with x < 2 (x is the slowest coordinate)
    rows = op.vals.size // op.vol
    cii = [torch.from_numpy(op.ii[c * half:(c + 1) * half].copy()).to(gpu) for c in range(2)]
    cjj = [torch.from_numpy(op.jj[c * half * op.nb:(c + 1) * half * op.nb].reshape(-1).copy()).to(gpu)
           for c in range(2)]
    cv = [device_values(to_half(op.vals[c * half * rows:(c + 1) * half * rows]), True, gpu)[0]
          for c in range(2)]
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


def test_half_powers(gpu):
    """y[p] = A^(p+1) x for p = 0, 1 on a square 16x16 operator: the first power's image pieces
    become the second one's x, all in complex<float>.  A component of A x is at most
    5 * 16 * 2 * 36 = 5760 in size and one of A^2 x at most 5 * 16 * 2 * 6 * 5760 < 2^23: exact."""
    import torch
    import superbblas_amd as sb
    b, ncols = 16, 12
    op = Op(LAT, b, b, C64)
    x = int_valued(op.vol * b * ncols, C64, 2)
    zero = np.zeros(op.vol * b * ncols, C64)
    y1 = reference(op, x, zero, ncols)
    y2 = reference(op, y1, zero, ncols)
    ox, dimx = layout(LAT, b, ncols, True, True)
    oy, _ = layout(LAT, b, ncols, True, False)
    dimy = [2] + dimx[1:]
    h = create(op, gpu)
    ty = torch.from_numpy(sentinel(2 * op.vol * b * ncols, C64)).to(gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                  "p", [ty])
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (FORM, 1), (form, mixed)
    assert np.array_equal(ty.cpu().numpy(), np.concatenate([y1, y2]))


@pytest.mark.parametrize("dtype", [C64, F32])
@pytest.mark.parametrize("key,value", [("mixed", 0), ("blk_mfma", 0), ("variant", 1)])
def test_half_switches(gpu, key, value, dtype):
    """each switch sends the product to the generic mixed form: the same exact result"""
    bi = bd = 48
    ncols = 12
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y1, form1, mixed1 = run(gpu, op, h, x, y0, ncols)
    with tuned(**{key: value}):
        y0_, form0, mixed0 = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form1, mixed1, form0, mixed0) == (FORM, 1, 0, 1)
    assert np.array_equal(y1, ref) and np.array_equal(y0_, ref)


@pytest.mark.parametrize("bi,bd,ncols,by_default", [(16, 16, 1, 0), (16, 16, 4, FORM), (24, 24, 4, 0),
                                                    (24, 24, 12, FORM), (32, 32, 1, FORM)])
def test_half_column_bound(gpu, bi, bd, ncols, by_default):
    """The default dispatch keeps 16x16 blocks with fewer than 4 rhs columns, and larger blocks
    of fewer than 1024 elements with fewer than 12, on the generic mixed form (where the
    matrix-core form was measured no faster); "bsr.blk_mfma" 2 takes them anyway, with the same
    exact result."""
    op = Op(LAT, bi, bd, C64)
    x = int_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu)
    y1, form1, _ = run(gpu, op, h, x, y0, ncols)
    with tuned(blk_mfma=2):
        y2, form2, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (form1, form2) == (by_default, FORM)
    assert np.array_equal(y1, ref) and np.array_equal(y2, ref)


@pytest.mark.parametrize("spin,color", [(1, 3), (2, 3), (4, 3)])
def test_half_small_blocks(gpu, spin, color):
    """3x3, 6x6 and 12x12 operators in complex32 with complex<float> vectors: the generic mixed
    form (their specialised kernels are one type throughout)"""
    import torch
    import superbblas_amd as sb
    from test_gpu_bsr import lattice_operator
    L, ncols = 4, 3
    dim, ii, jj, vals, nb = lattice_operator(L, spin, color, C64)
    b, vol = spin * color, L ** 4
    h16 = to_half(vals)
    assert np.array_equal(widened(h16, True), vals)
    x = int_valued(vol * b * ncols, C64, 2)
    ref = np.zeros(vol * b * ncols, C64)
    oracle_bsr(TYPE_OF[np.dtype(C64)], dim, 0, vol, b, b, ii, jj, vals, False, x, ncols, True, ref,
               ncols, True, ncols, 1.0)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, spin, color]
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj).to(gpu)], [device_values(h16, True, gpu)[0]])
    dimx = [1, L, L, L, L, spin, color, ncols]
    ty = torch.full((vol * b * ncols,), 7.0, dtype=torch.complex64, device=gpu)
    sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx,
                  [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                  dimx, "p", [ty])
    torch.cuda.synchronize()
    form, mixed = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")
    h.destroy()
    assert (form, mixed) == (0, 1), (form, mixed)
    assert np.array_equal(ty.cpu().numpy(), ref)


@pytest.mark.parametrize("mixed_key", [1, 0])
def test_half_values_read_in_place(gpu, mixed_key):
    """the operator reads the caller's value tensor at every product: scaled by 2 on the device
    (through its float16 view: exact) after the first product, the second product is twice the
    first (no converted copy is kept)"""
    import torch
    bi = bd = 48
    ncols = 12
    op = Op(LAT, bi, bd, C64)
    tv, t16 = device_values(to_half(op.vals), True, gpu)
    x = int_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    ref = reference(op, x, y0, ncols)
    h = create(op, gpu, values=tv)
    with tuned(mixed=mixed_key):
        y1, form1, _ = run(gpu, op, h, x, y0, ncols)
        t16.mul_(2)
        torch.cuda.synchronize()
        y2, form2, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert form1 == form2 == (FORM if mixed_key else 0)
    assert np.array_equal(y1, ref) and np.array_equal(y2, 2 * ref)


def random_half_op(bi, bd):
    """random values in [-1, 1] rounded to binary16 on the host; op.vals holds them widened"""
    op = Op(LAT, bi, bd, C64, values=random_valued)
    h16 = to_half(op.vals)
    op.vals = widened(h16, True)
    return op, h16


def test_half_accuracy(gpu):
    """Random data in [-1, 1] rounded to binary16 on the host, 64x64 complex32 blocks, five per
    row, 12 columns of complex<float> x, against numpy complex128 from the widened values.  Gate:
    the inner-product forward bound in FP32 for any summation order, the derivation of
    test_gpu_bsr_mixed.test_mixed_accuracy with u = 2^-24:
    ||y - y64||_2 / || |A| |x| ||_2 <= 2 (2 nb bd + 4) 2^-24 = 7.68e-5, for both forms.  The
    widening adds nothing to it (exact); a value flushed or rounded again on the way would.
    Measured on the MI355X: 2.891e-08 (matrix-core form) and 2.882e-08 (generic form)."""
    bi = bd = 64
    ncols = 12
    op, h16 = random_half_op(bi, bd)
    x = random_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    cols = np.ravel_multi_index(tuple(op.sites[..., d] for d in range(4)), op.lat)  # [vol, nb]
    A = op.vals.reshape(op.vol, op.nb, bi, bd).astype(np.complex128)
    X = x.astype(np.complex128).reshape(op.vol, bd, ncols)[cols]                    # [vol, nb, bd, n]
    y64 = np.einsum("rjab,rjbn->ran", A, X).reshape(-1)
    scale = np.linalg.norm(np.einsum("rjab,rjbn->ran", np.abs(A), np.abs(X)))
    gate = 2 * (2 * op.nb * bd + 4) * 2.0 ** -24
    h = create(op, gpu, values=device_values(h16, True, gpu)[0])
    y1, f1, m1 = run(gpu, op, h, x, y0, ncols)
    with tuned(mixed=0):
        yg, fg, mg = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    e1 = np.linalg.norm(y1 - y64) / scale
    eg = np.linalg.norm(yg - y64) / scale
    msg = "matrix-core form err %.3e, generic form err %.3e, gate %.3e" % (e1, eg, gate)
    print(msg)
    assert (f1, m1, fg, mg) == (FORM, 1, 0, 1), (f1, m1, fg, mg)
    assert e1 <= gate and eg <= gate, msg


def test_half_deterministic(gpu):
    bi = bd = 64
    ncols = 12
    op, h16 = random_half_op(bi, bd)
    x = random_valued(op.vol * bd * ncols, C64, 2)
    y0 = sentinel(op.vol * bi * ncols, C64)
    h = create(op, gpu, values=device_values(h16, True, gpu)[0])
    ya, fa, _ = run(gpu, op, h, x, y0, ncols)
    yb, fb, _ = run(gpu, op, h, x, y0, ncols)
    h.destroy()
    assert (fa, fb) == (FORM, FORM)
    assert np.array_equal(ya.view(np.uint8), yb.view(np.uint8))


def half_tensor(a, gpu):
    """a float32 / complex64 host array as (a float16 / complex32 device tensor, its float16 view)"""
    return device_values(to_half(a), a.dtype.kind == "c", gpu)


@pytest.mark.parametrize("vt,xt", [(C64, C128), (F32, F64), (C64, "half"), (F32, "half"), (F32, C64),
                                   (C64, F32)])
def test_half_refused_pairs(gpu, vt, xt):
    """a half-precision operator with double vectors, with half vectors, or real with complex
    vectors (and the reverse) keeps raising, and y keeps its sentinel"""
    import torch
    import superbblas_amd as sb
    bi = bd = 16
    ncols = 12
    op = Op(LAT, bi, bd, vt)
    h = create(op, gpu)
    ox, dimx = layout(LAT, bd, ncols, True, True)
    oy, dimy = layout(LAT, bi, ncols, True, False)
    if xt == "half":
        tx, _ = half_tensor(int_valued(op.vol * bd * ncols, vt, 2), gpu)
        ty, ty16 = half_tensor(sentinel(op.vol * bi * ncols, vt), gpu)
        want = to_half(sentinel(op.vol * bi * ncols, vt))
    else:
        tx = torch.from_numpy(int_valued(op.vol * bd * ncols, xt, 2)).to(gpu)
        ty = torch.from_numpy(sentinel(op.vol * bi * ncols, xt)).to(gpu)
        want = sentinel(op.vol * bi * ncols, xt)
    try:
        with pytest.raises(sb.SuperbblasError):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx, [tx],
                          0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy, "p", [ty])
        torch.cuda.synchronize()
    finally:
        h.destroy()
    got = ty16.cpu().numpy() if xt == "half" else ty.cpu().numpy()
    assert np.array_equal(got, want)


def test_half_refused_kronecker(gpu):
    """create_kron_bsr refuses half-precision values"""
    import torch
    import superbblas_amd as sb
    from test_gpu_kron_bsr import kron_lattice
    L, spin, color = 4, 4, 3
    ii, jj, vals, kron = kron_lattice(L, spin, color)
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
    with pytest.raises(sb.SuperbblasError, match="unsupported type"):
        sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False,
                           [torch.from_numpy(ii).to(gpu)], [torch.from_numpy(jj).to(gpu)],
                           [half_tensor(vals.astype(C64), gpu)[0]],
                           [half_tensor(kron.astype(C64), gpu)[0]])


@pytest.mark.parametrize("dtype", [C64, F32])
def test_half_refused_elsewhere(gpu, dtype):
    """copy, contraction, xgemm_batch_strided, cholesky and create_storage keep refusing float16 /
    complex32 tensors, with their "unsupported type" / "unsupported dtype" errors, and write
    nothing"""
    import torch
    import superbblas_amd as sb
    n = 8
    a, _ = half_tensor(int_valued(n * n, dtype, 1), gpu)
    b, _ = half_tensor(int_valued(n * n, dtype, 2), gpu)
    r, r16 = half_tensor(sentinel(n * n, dtype), gpu)
    want = to_half(sentinel(n * n, dtype))
    p = [([0, 0], [n, n])]
    unsupported = "unsupported (d)?type"
    with pytest.raises(sb.SuperbblasError, match=unsupported):
        sb.copy(1.0, p, "ab", [0, 0], [n, n], [n, n], [a], p, "ba", [0, 0], [n, n], [r])
    with pytest.raises(sb.SuperbblasError, match=unsupported):
        sb.contraction(1.0, p, [0, 0], [n, n], [n, n], "ab", False, [a], p, [0, 0], [n, n], [n, n],
                       "bc", False, [b], 0.0, p, [0, 0], [n, n], [n, n], "ac", [r])
    with pytest.raises(sb.SuperbblasError, match=unsupported):
        sb.xgemm_batch_strided("N", "N", n, n, n, 1.0, a, n, n * n, b, n, n * n, 0.0, r, n, n * n, 1)
    with pytest.raises(sb.SuperbblasError, match=unsupported):
        sb.cholesky(p, [n, n], "ab", [r], "a", "b")
    torch.cuda.synchronize()
    assert np.array_equal(r16.cpu().numpy(), want)
    with pytest.raises(sb.SuperbblasError, match=unsupported):
        sb.create_storage([n, n], sb.SlowToFast, "/nonexistent/half.s3t",
                          dtype=torch.complex32 if np.dtype(dtype).kind == "c" else torch.float16)
