"""Mixed-precision bsr_krylov on 12x12 (spin x colour) blocks -- the lattice's fine operator -- on
the 12x12 matrix-core kernels (kernels_bsr.hip): complex32 -> complex<float>, float16 -> float,
complex<float> -> complex<double> and float -> double.  The values are read in place in the
operator's type and widened where they are loaded; "bsr.last_kernel" reads the forms those kernels
have for same-type products (7 blocks by LDS-DMA, 8 the same with packed slots, 10 fragment
gathers with 9 blocks per row, 11 generic rows) and "bsr.last_mixed" 1.  From
"bsr.mixed12_min_cols" (4) rhs columns on; fewer columns, and "bsr.mixed" 0, stay on the generic
mixed form (0).

Exact against the oracle's builtin BSR loop in the vectors' type on the widened values:
lattice_operator's values (|re| <= 3, |im| <= 4) are exact in binary16, x components are at most 4
in size, a product component at most 3 * 4 + 4 * 4 = 28 and a row sum at most 9 * 12 * 28 = 3024,
times |alpha| components <= 2 and plus an integer y0: far below 2^24, so every sum is exact in
float in any order.  Lattices: L = 4 (256 rows) and L = 3 (81 rows: the LDS-DMA kernel's workgroup
holds 4 rows, the last one a single row)."""
import functools

import numpy as np
import pytest

from _common import TYPE_OF, int_valued, oracle_bsr, oracle_bsr_adjoint, random_valued
from test_gpu_bsr import lattice_operator
from test_gpu_bsr_half import SPECIAL_BITS, device_values, to_half, tuned, widened

pytestmark = pytest.mark.gpu

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
SPIN, COLOR, B, NB = 4, 3, 12, 9
# pair: (the values' type widened to a numpy type, stored as binary16, the vectors' type)
PAIRS = {"c32": (C64, True, C64), "f16": (F32, True, F32), "cf": (C64, False, C128),
         "f": (F32, False, F64)}
DMA, ELL, PF = (7, 8), (10,), (11,)
MATRIX_CORES = DMA + ELL + PF


@functools.lru_cache(maxsize=None)
def operator(L, vt):
    """lattice_operator's 9-point 12x12 operator: (dim, ii, jj [vol * 9, 6], vals); read only"""
    dim, ii, jj, vals, nb = lattice_operator(L, SPIN, COLOR, vt)
    assert nb == NB
    for a in (ii, jj, vals):
        a.setflags(write=False)
    return dim, ii, jj.reshape(-1, 6), vals


def x_of(n, dtype, seed=0):
    """integer data, components at most 4 in size"""
    g = np.arange(n) + 31 * seed
    return ((g % 9 - 4) + (1j * (g % 5 - 2) if np.dtype(dtype).kind == "c" else 0)).astype(dtype)


def value_tensor(vals, half, gpu, lead=0):
    """the operator's values on the device in their own type: (tensor, its float16 view or None);
    lead: the tensor starts that many elements into its buffer, which ends with the last value"""
    import torch
    cplx = vals.dtype.kind == "c"
    if half:
        h16 = to_half(vals)
        assert np.array_equal(widened(h16, cplx), vals)
        return device_values(h16, cplx, gpu, lead)
    buf = torch.empty(vals.size + lead, dtype=getattr(torch, vals.dtype.name), device=gpu)
    t = buf[lead:]
    t.copy_(torch.from_numpy(np.array(vals)))
    return t, None


def create(L, ii, jj, tv, gpu, imf=False):
    import torch
    import superbblas_amd as sb
    dim = [L, L, L, L, SPIN, COLOR]
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, SPIN, COLOR]
    return sb.create_bsr(full, dim, full, dim, blk, blk, imf,
                         [torch.from_numpy(np.array(ii)).to(gpu)],
                         [torch.from_numpy(np.array(jj).reshape(-1)).to(gpu)], [tv])


def layout(L, ncols, row, upper):
    o = "XYZTSC" if upper else "xyztsc"
    if row:
        return "p" + o + "n", [1, L, L, L, L, SPIN, COLOR, ncols]
    return "pn" + o, [1, ncols, L, L, L, L, SPIN, COLOR]


def run(gpu, L, h, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, adjoint=False):
    """y = alpha A x + beta y0 (A^H x when adjoint: x carries the image labels); y on the host,
    "bsr.last_kernel" and "bsr.last_mixed\""""
    import torch
    import superbblas_amd as sb
    ox, dimx = layout(L, ncols, xrow, not adjoint)
    oy, dimy = layout(L, ncols, yrow, adjoint)
    ty = torch.from_numpy(y0.copy()).to(gpu)
    sb.bsr_krylov(alpha, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                  [torch.from_numpy(x.copy()).to(gpu)], beta, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                  "p", [ty])
    torch.cuda.synchronize()
    return ty.cpu().numpy(), sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed")


def reference(L, ii, jj, vals, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, imf=False):
    """the oracle's loop in the vectors' type on the widened values"""
    vol = L ** 4
    y = (beta * y0).astype(x.dtype)
    oracle_bsr(TYPE_OF[x.dtype], [L, L, L, L, SPIN, COLOR], 0, vol, B, B, np.ascontiguousarray(ii),
               np.ascontiguousarray(jj).reshape(-1), np.ascontiguousarray(vals.astype(x.dtype)), imf, x,
               ncols if xrow else vol * B, xrow, y, ncols if yrow else vol * B, yrow, ncols, alpha,
               add=True)
    return y


@functools.lru_cache(maxsize=None)
def full_reference(L, pair, ncols, xrow=True, yrow=True, imf=False):
    """(x, y0, A x) of the whole operator, alpha 1 and beta 0; read only"""
    vt, _, xt = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    x = x_of(L ** 4 * B * ncols, xt)
    y0 = np.full(L ** 4 * B * ncols, 7.0, xt)
    ref = reference(L, ii, jj, vals, x, y0, ncols, xrow, yrow, imf=imf)
    for a in (x, y0, ref):
        a.setflags(write=False)
    return x, y0, ref


def product(gpu, L, pair, ncols, xrow=True, yrow=True, imf=False, lead=0, **keys):
    """the whole operator applied under the tune keys: (y, form, mixed, the exact result)"""
    vt, half, _ = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    x, y0, ref = full_reference(L, pair, ncols, xrow, yrow, imf)
    tv, _ = value_tensor(vals, half, gpu, lead)
    h = create(L, ii, jj, tv, gpu, imf)
    with tuned(**keys):
        y, form, mixed = run(gpu, L, h, x, y0, ncols, xrow, yrow)
    h.destroy()
    return y, form, mixed, ref


# (L, columns, x row major, y row major, block_im_fast, tune keys, the forms admitted)
EXACT = [
    # the LDS-DMA form, partial column tiles; 81 rows: one row in the last workgroup
    # (by default with packed slots, 8, below 12 columns and unpacked ones, 7, from 12)
    (4, 4, True, True, False, {}, (8,)), (3, 5, True, True, True, {}, (8,)),
    (4, 11, True, True, False, {}, (8,)), (4, 12, True, True, True, {}, (7,)),
    (3, 13, True, True, False, {}, (7,)), (4, 16, True, True, False, {}, (7,)),
    (3, 12, True, False, False, {}, (7,)),
    (3, 12, True, True, False, {"blk_pd": 1}, DMA), (4, 13, True, True, True, {"blk_pd": 3}, DMA),
    (3, 16, True, True, False, {"blk_pd": 2}, DMA),
    # ... both slot forms: packed (8; 1 to 5 instructions per slot by the pair and the column
    # count: 4, 5, 10, 11, 15 and 16 columns are on either side of every step) and unpacked (7)
    (3, 4, True, True, False, {"mixed12_pack": 2}, (8,)),
    (3, 5, True, True, True, {"mixed12_pack": 2}, (8,)),
    (3, 10, True, False, False, {"mixed12_pack": 2}, (8,)),
    (3, 11, True, True, False, {"mixed12_pack": 2}, (8,)),
    (3, 15, True, True, True, {"mixed12_pack": 2, "blk_pd": 2}, (8,)),
    (4, 16, True, True, False, {"mixed12_pack": 2, "blk_pd": 3}, (8,)),
    (3, 1, True, True, False, {"mixed12_pack": 2, "mixed12_min_cols": 1}, (8,)),
    (3, 4, True, True, True, {"mixed12_pack": 0}, (7,)),
    (4, 12, True, False, False, {"mixed12_pack": 0}, (7,)),
    (3, 16, True, True, False, {"mixed12_pack": 0, "blk_pd": 3}, (7,)),
    # fragment gathers: several column tiles, column-major x and y, variant 2
    (4, 17, True, True, False, {}, ELL), (3, 20, True, True, True, {}, ELL),
    (3, 40, True, True, False, {}, ELL), (4, 12, False, False, False, {}, ELL),
    (3, 5, False, True, True, {}, ELL), (4, 12, True, True, True, {"variant": 2}, ELL),
    (3, 20, True, False, False, {"variant": 2}, ELL),
    # generic rows: variant 1
    (4, 12, True, True, False, {"variant": 1}, PF), (3, 17, False, True, True, {"variant": 1}, PF),
]


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("L,ncols,xrow,yrow,imf,keys,forms", EXACT)
def test_mixed12_exact(gpu, pair, L, ncols, xrow, yrow, imf, keys, forms):
    y, form, mixed, ref = product(gpu, L, pair, ncols, xrow, yrow, imf, **keys)
    assert form in forms and mixed == 1, (form, mixed)
    assert y.dtype == ref.dtype and np.array_equal(y, ref)


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("ncols,keys,forms", [(12, {}, DMA), (20, {}, ELL), (5, {"variant": 1}, PF)])
def test_mixed12_alpha_beta(gpu, pair, ncols, keys, forms):
    """alpha = 2 - i (2 for the real pairs) and beta = 1 against an integer y0"""
    L = 3
    vt, half, xt = PAIRS[pair]
    alpha = 2 - 1j if np.dtype(xt).kind == "c" else 2.0
    _, ii, jj, vals = operator(L, vt)
    x = x_of(L ** 4 * B * ncols, xt)
    y0 = int_valued(L ** 4 * B * ncols, xt, 3)
    ref = reference(L, ii, jj, vals, x, y0, ncols, alpha=alpha, beta=1.0)
    h = create(L, ii, jj, value_tensor(vals, half, gpu)[0], gpu)
    with tuned(**keys):
        y, form, mixed = run(gpu, L, h, x, y0, ncols, alpha=alpha, beta=1.0)
    h.destroy()
    assert form in forms and mixed == 1, (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pair", ["c32", "cf"])
@pytest.mark.parametrize("ncols", [1, 3])
def test_mixed12_column_bound(gpu, pair, ncols):
    """fewer than "bsr.mixed12_min_cols" (4) columns: the generic mixed form by default, a
    matrix-core form with the bound at 1; the same exact result"""
    y0, form0, mixed0, ref = product(gpu, 3, pair, ncols)
    y1, form1, mixed1, _ = product(gpu, 3, pair, ncols, mixed12_min_cols=1)
    assert (form0, mixed0, mixed1) == (0, 1, 1) and form1 in MATRIX_CORES, (form0, form1)
    assert np.array_equal(y0, ref) and np.array_equal(y1, ref)


@pytest.mark.parametrize("pair", ["c32", "cf"])
def test_mixed12_switch(gpu, pair):
    """"bsr.mixed" 0: the generic mixed form at 12 columns"""
    y, form, mixed, ref = product(gpu, 3, pair, 12, mixed=0)
    assert (form, mixed) == (0, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pd,pack", [(1, 2), (3, 2), (1, 0), (3, 0)])
@pytest.mark.parametrize("pair,ncols", [("c32", 13), ("c32", 16), ("cf", 12)])
def test_mixed12_skipped_blocks_dma(gpu, pair, ncols, pd, pack):
    """test_bsr_12x12_skipped_blocks_dma's pattern on the LDS-DMA form: column -1 on every third
    row's second block, on the very last block of the value array and on a whole row; the value and
    x tensors exactly as long as the operator needs (the values' buffer ends with the last block, x
    is vol * 12 * ncols elements).  A skipped block's slot must not read past either array and must
    add nothing.  Packed slots (form 8: a 16-column complex<float> x block is longer than a
    complex32 value block, so a slot's x part of the last block would run past the values if it were
    read from them) and unpacked ones (7)."""
    L = 4
    vt, half, xt = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    vol = L ** 4
    jj = jj.reshape(vol, NB, 6).copy()
    jj[::3, 1, :] = -1
    jj[-1, NB - 1, :] = -1
    jj[-2, :, :] = -1
    x = x_of(vol * B * ncols, xt)
    y0 = np.full(vol * B * ncols, 3.0, xt)
    ref = reference(L, ii, jj, vals, x, y0, ncols)
    tv, _ = value_tensor(vals, half, gpu)
    assert tv.numel() == vol * NB * B * B
    h = create(L, ii, jj, tv, gpu)
    with tuned(blk_pd=pd, mixed12_pack=pack):
        y, form, mixed = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (8 if pack else 7, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pair,ncols", [("c32", 12), ("f16", 5), ("cf", 17), ("f", 12)])
def test_mixed12_ragged_rows(gpu, pair, ncols):
    """row r keeps its first r mod 10 blocks (a CSR operator): the generic rows, form 11"""
    L = 3
    vt, half, xt = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    vol = L ** 4
    keep = np.arange(vol) % (NB + 1)
    sel = np.concatenate([np.arange(r * NB, r * NB + keep[r], dtype=np.int64) for r in range(vol)])
    ii2 = keep.astype(np.int32)
    jj2 = np.ascontiguousarray(jj[sel])
    vals2 = np.ascontiguousarray(vals.reshape(-1, B * B)[sel]).reshape(-1)
    x = x_of(vol * B * ncols, xt)
    y0 = np.full(vol * B * ncols, 7.0, xt)
    ref = reference(L, ii2, jj2, vals2, x, y0, ncols)
    h = create(L, ii2, jj2, value_tensor(vals2, half, gpu)[0], gpu)
    y, form, mixed = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    assert (form, mixed) == (11, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pair,align", [("c32", 4), ("f16", 2), ("cf", 8), ("f", 4)])
def test_mixed12_unaligned_values(gpu, pair, align):
    """the value tensor starts one element into its buffer, so it is no 16-byte multiple from any
    16-byte boundary: the LDS-DMA form moves 16-byte pieces and is not taken; the fragment gathers
    read the values by elements"""
    vt, half, _ = PAIRS[pair]
    tv, _ = value_tensor(operator(3, vt)[3], half, gpu, lead=1)
    assert tv.data_ptr() % 16 == align
    y, form, mixed, ref = product(gpu, 3, pair, 12, lead=1)
    assert form in ELL + PF and mixed == 1, (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pair", ["c32", "f16"])
@pytest.mark.parametrize("keys,forms", [({}, DMA), ({"variant": 2}, ELL), ({"variant": 1}, PF)])
def test_mixed12_exact_widening(gpu, pair, keys, forms):
    """test_half_exact_widening's argument on 12x12 blocks: x holds the 12 unit vectors on site 0
    and zeros elsewhere, 12 columns, so a row's only block on site 0 appears in y widened and every
    other term of every sum is a zero -- no rounding anywhere.  The values cycle through 65504,
    -65504, 2^-14, 2^-24, subnormals with several mantissa bits and +-0."""
    L, ncols = 3, B
    vt, _, xt = PAIRS[pair]
    cplx = np.dtype(vt).kind == "c"
    _, ii, jj, _ = operator(L, vt)
    vol = L ** 4
    n16 = vol * NB * B * B * (2 if cplx else 1)
    h16 = SPECIAL_BITS[(np.arange(n16) * 5 + np.arange(n16) // 7) % SPECIAL_BITS.size].view(np.float16)
    vals = widened(h16, cplx)
    assert np.all(np.isfinite(vals.view(np.float32)))
    assert np.float32(2.0 ** -24) in vals.view(np.float32) and np.float32(65504) in vals.view(np.float32)
    x = np.zeros((vol * B, ncols), xt)
    x[np.arange(B), np.arange(B)] = 1
    x = x.reshape(-1)
    y0 = np.full(vol * B * ncols, 7.0, xt)
    ref = reference(L, ii, jj, vals, x, y0, ncols)
    # the reference is itself a copy of blocks: row 0's first block is the site's own
    assert np.array_equal(ref.reshape(vol, B, ncols)[0], vals.reshape(vol, NB, B, B)[0, 0])
    h = create(L, ii, jj, device_values(h16, cplx, gpu)[0], gpu)
    with tuned(**keys):
        y, form, mixed = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    assert form in forms and mixed == 1, (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("ncols,forms", [(12, DMA), (20, ELL)])
def test_mixed12_values_read_in_place(gpu, ncols, forms):
    """the operator reads the caller's value tensor at every product: scaled by 2 on the device
    (through its float16 view: exact) after the first product, the second is twice the first"""
    import torch
    L, pair = 3, "c32"
    vt, half, _ = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    x, y0, ref = full_reference(L, pair, ncols)
    tv, t16 = value_tensor(vals, half, gpu)
    h = create(L, ii, jj, tv, gpu)
    y1, form1, mixed1 = run(gpu, L, h, x, y0, ncols)
    t16.mul_(2)
    torch.cuda.synchronize()
    y2, form2, mixed2 = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    assert form1 in forms and form2 == form1 and (mixed1, mixed2) == (1, 1), (form1, form2)
    assert np.array_equal(y1, ref) and np.array_equal(y2, 2 * ref)


@pytest.mark.parametrize("pair,per_element", [("c32", 4), ("f16", 2), ("cf", 8)])
def test_mixed12_adjoint(gpu, pair, per_element):
    """x with the image labels.  "bsr.adj_inplace" 0: A^H x through the conjugated, regrouped copy,
    which stays in the operator's type ("bsr.adj_copy_bytes" grows by the operator's bytes per
    element) and runs a 12x12 matrix-core form; "bsr.adj_inplace" 1 stays on the generic in-place
    form 18.  Exact against the oracle's adjoint loop."""
    import superbblas_amd as sb
    L, ncols = 3, 12
    vt, half, xt = PAIRS[pair]
    _, ii, jj, vals = operator(L, vt)
    vol = L ** 4
    x = x_of(vol * B * ncols, xt, 1)
    y0 = np.full(vol * B * ncols, 7.0, xt)
    ref = np.zeros(vol * B * ncols, xt)
    oracle_bsr_adjoint(TYPE_OF[np.dtype(xt)], [L, L, L, L, SPIN, COLOR], 0, vol, B, B, ii,
                       np.ascontiguousarray(jj).reshape(-1), np.ascontiguousarray(vals.astype(xt)), False,
                       x, ncols, True, ref, ncols, True, vol * B, ncols, 1.0)
    h = create(L, ii, jj, value_tensor(vals, half, gpu)[0], gpu)
    before = sb.tune_get("bsr.adj_copy_bytes")
    with tuned(adj_inplace=0):
        y, form, mixed = run(gpu, L, h, x, y0, ncols, adjoint=True)
    held = sb.tune_get("bsr.adj_copy_bytes") - before
    h.destroy()
    assert form in MATRIX_CORES and mixed == 1, (form, mixed)
    assert held == per_element * vals.size, (held, vals.size)
    assert sb.tune_get("bsr.adj_copy_bytes") == before
    assert np.array_equal(y, ref)
    h = create(L, ii, jj, value_tensor(vals, half, gpu)[0], gpu)
    with tuned(adj_inplace=1):
        y, form, mixed = run(gpu, L, h, x, y0, ncols, adjoint=True)
    h.destroy()
    assert (form, mixed) == (18, 1), (form, mixed)
    assert np.array_equal(y, ref)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_mixed12_accuracy(gpu, pair):
    """Random values in [-1, 1] rounded to binary16 (to float for the float -> double pairs) on the
    host, 12 columns of random x, against numpy complex128 / float64 from the widened values.
    Gate: the inner-product forward bound of test_half_accuracy for any summation order,
    ||y - y64||_2 / || |A| |x| ||_2 <= 2 (2 nb bd + 4) u with nb = 9, bd = 12: 2.62e-5 with
    u = 2^-24 (half pairs), 4.88e-14 with u = 2^-53 (float -> double pairs); for the LDS-DMA form
    and the generic mixed form alike.  The widening adds nothing to it (exact).
    Measured on the MI355X (LDS-DMA form / generic form): complex32 2.889e-08 / 2.885e-08, float16
    2.346e-08 / 2.346e-08, complex<float> 6.652e-17 / 6.637e-17, float 3.132e-17 / 3.132e-17."""
    L, ncols = 3, 12
    vt, half, xt = PAIRS[pair]
    _, ii, jj, _ = operator(L, vt)
    vol = L ** 4
    vals = random_valued(vol * NB * B * B, vt, 5)
    if half:
        h16 = to_half(vals)
        vals = widened(h16, np.dtype(vt).kind == "c")
        tv = device_values(h16, np.dtype(vt).kind == "c", gpu)[0]
    else:
        tv = value_tensor(vals, False, gpu)[0]
    x = random_valued(vol * B * ncols, xt, 2)
    y0 = np.full(vol * B * ncols, 7.0, xt)
    wide = np.complex128 if np.dtype(xt).kind == "c" else np.float64
    cols = np.ravel_multi_index(tuple(jj.reshape(vol, NB, 6)[..., d] for d in range(4)), (L,) * 4)
    A = vals.reshape(vol, NB, B, B).astype(wide)
    X = x.astype(wide).reshape(vol, B, ncols)[cols]  # [vol, nb, bd, n]
    y64 = np.einsum("rjab,rjbn->ran", A, X).reshape(-1)
    scale = np.linalg.norm(np.einsum("rjab,rjbn->ran", np.abs(A), np.abs(X)))
    gate = 2 * (2 * NB * B + 4) * (2.0 ** -24 if half else 2.0 ** -53)
    h = create(L, ii, jj, tv, gpu)
    y1, f1, m1 = run(gpu, L, h, x, y0, ncols)
    with tuned(mixed=0):
        yg, fg, mg = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    e1 = np.linalg.norm(y1 - y64) / scale
    eg = np.linalg.norm(yg - y64) / scale
    msg = "%s: matrix-core form err %.3e, generic form err %.3e, gate %.3e" % (pair, e1, eg, gate)
    print(msg)
    assert f1 in DMA and (m1, fg, mg) == (1, 0, 1), (f1, m1, fg, mg)
    assert e1 <= gate and eg <= gate, msg


@pytest.mark.parametrize("pair,ncols,forms", [("c32", 12, DMA), ("c32", 20, ELL), ("cf", 13, DMA)])
def test_mixed12_deterministic(gpu, pair, ncols, forms):
    L = 3
    vt, half, xt = PAIRS[pair]
    _, ii, jj, _ = operator(L, vt)
    vol = L ** 4
    vals = random_valued(vol * NB * B * B, vt, 5)
    if half:
        tv = device_values(to_half(vals), np.dtype(vt).kind == "c", gpu)[0]
    else:
        tv = value_tensor(vals, False, gpu)[0]
    x = random_valued(vol * B * ncols, xt, 2)
    y0 = np.full(vol * B * ncols, 7.0, xt)
    h = create(L, ii, jj, tv, gpu)
    ya, fa, ma = run(gpu, L, h, x, y0, ncols)
    yb, fb, mb = run(gpu, L, h, x, y0, ncols)
    h.destroy()
    assert fa in forms and fb == fa and (ma, mb) == (1, 1), (fa, fb)
    assert np.array_equal(ya.view(np.uint8), yb.view(np.uint8))
