"""A^H of plain BSR operators read from A's values in place ("bsr.adj_inplace" 1): bsr_krylov with
the image labels on x reads the value array of create_bsr through an entry list, conjugating at
the load -- bsr_blk_mfma_kernel's adjoint form ("bsr.last_kernel" 17) where the dense-block clause
would take the transposed copy, bsr_kernel's (18) otherwise -- so no second copy of the values exists
("bsr.adj_copy_bytes") and A^H follows the changes the caller makes to them.  With the key at its
default 0 nothing changes (the existing tests pin that; here only where a test needs both).

Exact against the oracle's adjoint loop on integer-valued data: components are at most 6, a
product component at most 61; on the (2,2,2,2) lattice a block column has 5 entries, so a column
sum is at most 5 * 128 * 61 = 39 040, times |alpha| <= 3 and after the values are doubled still
far below 2^24: exact in float32 in any order."""
import functools

import numpy as np
import pytest

from _common import TYPE_OF, int_valued, oracle_bsr, oracle_bsr_adjoint, random_valued
from test_gpu_bsr_blocks import Op, apply, layout, sentinel, split
from test_gpu_bsr_mixed import tuned

pytestmark = pytest.mark.gpu

MFMA, GENERIC, COPY_MFMA = 17, 18, 14
LAT = (2, 2, 2, 2)
C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
WIDE = {np.dtype(C64): np.dtype(C128), np.dtype(F32): np.dtype(F64)}


def adjoint_reference(op, x, y0, ncols, xrow=True, yrow=True, alpha=1.0, beta=0.0, im_fast=False):
    """alpha A^H x + beta y0 by the oracle's loop in x's type (the values up-converted for the
    mixed pairs, exactly)"""
    y = (beta * y0).astype(x.dtype)
    oracle_bsr_adjoint(TYPE_OF[x.dtype], op.dimd, 0, op.vol, op.bi, op.bd, op.ii, op.jj.reshape(-1),
                       op.vals.astype(x.dtype), im_fast, x, ncols if xrow else op.vol * op.bi, xrow, y,
                       ncols if yrow else op.vol * op.bd, yrow, op.vol * op.bd, ncols, alpha, add=True)
    return y


def create(op, gpu, im_fast=False, values=None):
    """create_bsr on the operator's arrays; values: a device tensor to use as it is"""
    import torch
    import superbblas_amd as sb
    pi, pd = [([0] * 6, op.dimi)], [([0] * 6, op.dimd)]
    tv = torch.from_numpy(op.vals).to(gpu) if values is None else values
    return sb.create_bsr(pi, op.dimi, pd, op.dimd, [1, 1, 1, 1] + list(split(op.bi)),
                         [1, 1, 1, 1] + list(split(op.bd)), im_fast,
                         [torch.from_numpy(op.ii).to(gpu)],
                         [torch.from_numpy(op.jj.reshape(-1)).to(gpu)], [tv])


def real_if(dtype, alpha):
    return alpha if np.dtype(dtype).kind == "c" else alpha.real


# a pairwise-covering subset of (block) x (type) x (columns) x (x layout) x (y layout) x
# (block_im_fast): every block with two types or more, every type with a non-square block, rows
# that are no 16-byte multiple ((18,22) and, read transposed, the column runs of every
# row-major operator) and each of the column counts 1, 3, 12, 16, 17, 40 (partial tiles, one, two
# and four column tiles per workgroup); A^H of a bi x bd operator has bd x bi blocks: strips of
# one (16), two (18-32) and more rows, up to the launcher's 128
EXACT = [
    (16, 16, C64, 16, True, True, False), (16, 16, F64, 3, False, True, True),
    (16, 16, C128, 40, True, False, False), (24, 24, C128, 12, True, False, False),
    (24, 24, F32, 17, False, False, True), (24, 24, C64, 1, True, True, True),
    (48, 48, C64, 12, True, True, False), (48, 48, C128, 3, True, True, True),
    (48, 48, F64, 40, True, False, False), (64, 64, C64, 16, True, True, False),
    (64, 64, C128, 40, False, True, False), (64, 64, F32, 1, True, True, True),
    (20, 36, C64, 17, False, False, True), (20, 36, C128, 12, True, True, False),
    (36, 20, F32, 40, True, True, False), (36, 20, C128, 3, False, True, True),
    (36, 20, C64, 16, True, False, False), (18, 22, C64, 17, True, False, False),
    (18, 22, F32, 12, True, True, False), (18, 22, F64, 40, False, True, True),
    (18, 22, C128, 1, False, False, False), (32, 16, C64, 40, True, True, True),
    (32, 16, F64, 12, True, True, False), (16, 80, C128, 17, True, True, False),
    (16, 80, F32, 16, False, False, False), (128, 128, C128, 12, True, True, False),
    (128, 128, C64, 17, False, True, True), (128, 128, F32, 1, True, False, True),
]


@pytest.mark.parametrize("bi,bd,dtype,ncols,xrow,yrow,imf", EXACT)
def test_adjoint_inplace_exact(gpu, bi, bd, dtype, ncols, xrow, yrow, imf):
    """both forms, with a complex alpha and beta = 2 over a pre-filled y and with beta = 0 over a
    sentinel; the generic form through "bsr.blk_mfma" 0 or "bsr.variant" 1 (alternating)"""
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    alpha = real_if(dtype, 2 - 1j)
    filled, sent = int_valued(op.vol * bd * ncols, dtype, 3), sentinel(op.vol * bd * ncols, dtype)
    ref2 = adjoint_reference(op, x, filled, ncols, xrow, yrow, alpha, 2.0, imf)
    ref0 = adjoint_reference(op, x, sent, ncols, xrow, yrow, alpha, 0.0, imf)
    off = {"blk_mfma": 0} if (bi + ncols) % 2 else {"variant": 1}
    h = create(op, gpu, imf)
    out = {}
    try:
        for form, keys in ((MFMA, {"blk_mfma": 2}), (GENERIC, off)):
            with tuned(adj_inplace=1, **keys):
                out[form, 2] = apply(gpu, op, h, x, filled, ncols, xrow, yrow, alpha, 2.0, adjoint=True)
                out[form, 0] = apply(gpu, op, h, x, sent, ncols, xrow, yrow, alpha, 0.0, adjoint=True)
    finally:
        h.destroy()
    for (form, beta), (y, used) in out.items():
        assert used == form, (form, beta, used)
        assert np.array_equal(y, ref2 if beta else ref0), (form, beta)


@pytest.mark.parametrize("bi,bd,ncols,form", [(16, 16, 4, GENERIC), (16, 16, 12, MFMA),
                                              (24, 24, 1, GENERIC), (32, 32, 1, MFMA)])
def test_adjoint_inplace_column_bound(gpu, bi, bd, ncols, form):
    """with "bsr.blk_mfma" at its default 1 the in-place adjoint follows the dense-block clause's
    column thresholds: what it declines runs the generic in-place form"""
    import superbblas_amd as sb
    assert sb.tune_get("bsr.blk_mfma") == 1 and sb.tune_get("bsr.blk_min") == 16
    op = Op(LAT, bi, bd, C128)
    x = int_valued(op.vol * bi * ncols, C128, 2)
    y0 = sentinel(op.vol * bd * ncols, C128)
    ref = adjoint_reference(op, x, y0, ncols)
    h = create(op, gpu)
    try:
        with tuned(adj_inplace=1):
            y, used = apply(gpu, op, h, x, y0, ncols, adjoint=True)
    finally:
        h.destroy()
    assert used == form, used
    assert np.array_equal(y, ref)


def referenced_columns(op):
    """the block columns (sites) that a block of the operator points at"""
    jj = op.jj.reshape(-1, 6)
    kept = jj[jj[:, 0] >= 0]
    return set(np.ravel_multi_index(tuple(kept[:, d] for d in range(4)), op.lat).tolist())


@pytest.mark.parametrize("pattern", ["ragged", "skipped"])
@pytest.mark.parametrize("bi,bd,dtype,ncols", [(48, 48, C64, 13), (20, 36, C128, 5), (18, 22, F32, 16)])
def test_adjoint_inplace_patterns(gpu, bi, bd, dtype, ncols, pattern):
    """The two patterns of test_blocks_ragged_and_skipped, each made to leave one block column
    that nothing points at.  ragged: row r keeps r mod (nb + 1) blocks, rows 4 and 8 fewer, so
    that no kept block points at site 0 (row 0 keeps none; its neighbours 1, 2, 4, 8 point at it
    with their blocks 4, 3, 2, 1).  skipped: column -1 on every third row's second block, on the
    last block of the value array, on a whole row and on every block that points at site 5.  The
    block columns then have different entry counts; the empty one reads beta y0 (0 for beta = 0,
    never the sentinel).  Both forms."""
    op = Op(LAT, bi, bd, dtype)
    if pattern == "ragged":
        counts = np.arange(op.vol) % (op.nb + 1)
        counts[8], counts[4] = 1, 2
        op.keep(counts)
        empty = 0
    else:
        jj = op.jj.reshape(op.vol, op.nb, 6)
        jj[::3, 1, :] = -1
        jj[-1, op.nb - 1, :] = -1
        jj[-2, :, :] = -1
        cols = np.ravel_multi_index(tuple(op.sites[..., d] for d in range(4)), op.lat)
        jj[cols == 5] = -1
        empty = 5
    refd = referenced_columns(op)
    assert empty not in refd and len(refd) > op.vol // 2
    assert op.vals.size == int(op.ii.sum()) * bi * bd
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    alpha = real_if(dtype, 1 - 2j)
    filled, sent = int_valued(op.vol * bd * ncols, dtype, 3), sentinel(op.vol * bd * ncols, dtype)
    ref2 = adjoint_reference(op, x, filled, ncols, alpha=alpha, beta=2.0)
    ref0 = adjoint_reference(op, x, sent, ncols, alpha=alpha)
    rows = slice(empty * bd * ncols, (empty + 1) * bd * ncols)
    assert np.array_equal(ref2[rows], 2 * filled[rows]) and not ref0[rows].any()
    h = create(op, gpu)
    out = {}
    try:
        for form, mfma in ((MFMA, 2), (GENERIC, 0)):
            with tuned(adj_inplace=1, blk_mfma=mfma):
                out[form, 2] = apply(gpu, op, h, x, filled, ncols, alpha=alpha, beta=2.0, adjoint=True)
                out[form, 0] = apply(gpu, op, h, x, sent, ncols, alpha=alpha, adjoint=True)
    finally:
        h.destroy()
    for (form, beta), (y, used) in out.items():
        assert used == form, (form, beta, used)
        assert np.array_equal(y, ref2 if beta else ref0), (form, beta)


def test_adjoint_inplace_unaligned_values(gpu):
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
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    h = create(op, gpu, im_fast=True, values=tv)  # (read transposed: row-major blocks for A^H)
    try:
        with tuned(adj_inplace=1):
            y, used = apply(gpu, op, h, x, y0, ncols, adjoint=True)
    finally:
        h.destroy()
    assert used == MFMA, used
    assert np.array_equal(y, adjoint_reference(op, x, y0, ncols, im_fast=True))


@pytest.mark.parametrize("spin,color,ncols,by_copy", [(1, 3, 12, 2), (1, 3, 2, 1), (4, 3, 3, 7)])
def test_adjoint_inplace_small_blocks(gpu, spin, color, ncols, by_copy):
    """3x3 and 12x12 operators: the generic in-place form with the key at 1 (their LDS-DMA kernels
    stream contiguous value runs), their own kernels on the copy with the key at 0, as ever"""
    import torch
    import superbblas_amd as sb
    from test_gpu_bsr import lattice_operator
    L = 4
    dim, ii, jj, vals, nb = lattice_operator(L, spin, color)
    b, vol = spin * color, L ** 4
    n = vol * b * ncols
    x = int_valued(n, C128, 2)
    ref = np.zeros(n, C128)
    oracle_bsr_adjoint(TYPE_OF[np.dtype(C128)], dim, 0, vol, b, b, ii, jj, vals, False, x, ncols, True,
                       ref, ncols, True, vol * b, ncols, 1.0)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, spin, color]
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj).to(gpu)], [torch.from_numpy(vals).to(gpu)])
    dimx = [1, L, L, L, L, spin, color, ncols]
    tx = torch.from_numpy(x).to(gpu)
    got = {}
    try:
        for key in (1, 0):
            ty = torch.full((n,), 7.0, dtype=torch.complex128, device=gpu)
            with tuned(adj_inplace=key):
                sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                              dimx, [tx], 0.0, [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx,
                              "p", [ty])
                torch.cuda.synchronize()
                got[key] = (ty.cpu().numpy(), sb.tune_get("bsr.last_kernel"))
    finally:
        h.destroy()
    assert (got[1][1], got[0][1]) == (GENERIC, by_copy)
    assert np.array_equal(got[1][0], ref) and np.array_equal(got[0][0], ref)


@pytest.mark.parametrize("bi,bd,dtype,ncols,xrow,yrow,imf", [
    (48, 48, C64, 12, True, True, False), (20, 36, F32, 17, False, True, True),
    (18, 22, C64, 3, True, False, True), (64, 64, F32, 16, True, True, False)])
def test_adjoint_inplace_mixed_pairs(gpu, bi, bd, dtype, ncols, xrow, yrow, imf):
    """single-precision values with vectors of the double counterpart: the generic in-place form
    (also where "bsr.blk_mfma" 2 asks for the matrix cores), y in the double type"""
    import superbblas_amd as sb
    op = Op(LAT, bi, bd, dtype)
    wt = WIDE[op.dtype]
    x = int_valued(op.vol * bi * ncols, wt, 2)
    y0 = sentinel(op.vol * bd * ncols, wt)
    ref = adjoint_reference(op, x, y0, ncols, xrow, yrow, im_fast=imf)
    h = create(op, gpu, imf)
    try:
        with tuned(adj_inplace=1, blk_mfma=2):
            y, used = apply(gpu, op, h, x, y0, ncols, xrow, yrow, adjoint=True)
            mixed = sb.tune_get("bsr.last_mixed")
    finally:
        h.destroy()
    assert (used, mixed) == (GENERIC, 1), (used, mixed)
    assert y.dtype == wt and np.array_equal(y, ref)


@pytest.mark.parametrize("form,blk_mfma", [(MFMA, 2), (GENERIC, 0)])
def test_adjoint_inplace_follows_the_values(gpu, form, blk_mfma):
    """A^H reads the caller's value tensor at every product, as A does: scaled by 2 on the device
    after the first product, the second product is twice the first"""
    import torch
    bi, bd, ncols = 48, 32, 12
    op = Op(LAT, bi, bd, C64)
    tv = torch.from_numpy(op.vals).to(gpu)
    x = int_valued(op.vol * bi * ncols, C64, 2)
    y0 = sentinel(op.vol * bd * ncols, C64)
    ref = adjoint_reference(op, x, y0, ncols)
    h = create(op, gpu, values=tv)
    try:
        with tuned(adj_inplace=1, blk_mfma=blk_mfma):
            y1, f1 = apply(gpu, op, h, x, y0, ncols, adjoint=True)
            tv.mul_(2)
            torch.cuda.synchronize()
            y2, f2 = apply(gpu, op, h, x, y0, ncols, adjoint=True)
    finally:
        h.destroy()
    assert (f1, f2) == (form, form)
    assert np.array_equal(y1, ref) and np.array_equal(y2, 2 * ref)


def test_adjoint_inplace_makes_no_copy(gpu):
    """"bsr.adj_copy_bytes" stays where it is through the life of an operator only used with the
    key at 1; with the key at 0 the first A^H product adds the conjugated copy, exactly the
    non-skipped blocks, and destroy() gives it back"""
    import superbblas_amd as sb
    bi, bd, ncols, dtype = 48, 32, 12, C64
    op = Op(LAT, bi, bd, dtype)
    jj = op.jj.reshape(op.vol, op.nb, 6)
    jj[::3, 1, :] = -1
    kept = int((op.jj.reshape(-1, 6)[:, 0] >= 0).sum())
    assert 0 < kept < op.vol * op.nb
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, y0, ncols)
    before = sb.tune_get("bsr.adj_copy_bytes")
    seen = []
    h = create(op, gpu)
    try:
        seen.append(sb.tune_get("bsr.adj_copy_bytes"))
        with tuned(adj_inplace=1):
            for _ in range(3):
                y, used = apply(gpu, op, h, x, y0, ncols, adjoint=True)
                assert used == MFMA and np.array_equal(y, ref)
                seen.append(sb.tune_get("bsr.adj_copy_bytes"))
    finally:
        h.destroy()
    seen.append(sb.tune_get("bsr.adj_copy_bytes"))
    assert seen == [before] * 5, (before, seen)
    h = create(op, gpu)
    try:
        assert sb.tune_get("bsr.adj_copy_bytes") == before
        y, used = apply(gpu, op, h, x, y0, ncols, adjoint=True)
        assert used == COPY_MFMA and np.array_equal(y, ref)
        held = sb.tune_get("bsr.adj_copy_bytes")
        apply(gpu, op, h, x, y0, ncols, adjoint=True)
        again = sb.tune_get("bsr.adj_copy_bytes")
    finally:
        h.destroy()
    assert held - before == kept * bi * bd * np.dtype(dtype).itemsize, (held, before)
    assert again == held
    assert sb.tune_get("bsr.adj_copy_bytes") == before


@pytest.mark.parametrize("keys", [(1, 0, 1), (0, 1, 0)])
def test_adjoint_inplace_one_handle_both_settings(gpu, keys):
    """the key is read at each product and the two value sources are built independently, each
    at the first product that asks for it"""
    bi, bd, ncols, dtype = 48, 48, 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, y0, ncols)
    h = create(op, gpu)
    got = []
    try:
        for key in keys:
            with tuned(adj_inplace=key):
                got.append(apply(gpu, op, h, x, y0, ncols, adjoint=True))
    finally:
        h.destroy()
    assert [f for _, f in got] == [MFMA if key else COPY_MFMA for key in keys]
    for y, _ in got:
        assert np.array_equal(y, ref)


@pytest.mark.parametrize("bi,bd,dtype,ncols", [(64, 64, C64, 12), (20, 36, C128, 17)])
def test_adjoint_inplace_same_bits_as_the_copy(gpu, bi, bd, dtype, ncols):
    """Random values and x.  The conjugation is an exact sign flip, the entries go in the copy's
    order and the operand order is the copy form's, so the in-place forms reproduce the bits of
    the corresponding kernel on the copy: 17 against 14, 18 against the generic kernel
    ("bsr.variant" 1, form 0); no tolerance.  Two runs of each in-place form agree bit for bit."""
    op = Op(LAT, bi, bd, dtype, values=random_valued)
    x = random_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    h = create(op, gpu)
    got = {}
    try:
        for variant in (0, 1):
            for key in (1, 0, 1):
                with tuned(adj_inplace=key, variant=variant):
                    got.setdefault((variant, key), []).append(apply(gpu, op, h, x, y0, ncols, adjoint=True))
    finally:
        h.destroy()
    forms = {k: [f for _, f in v] for k, v in got.items()}
    assert forms == {(0, 1): [MFMA, MFMA], (0, 0): [COPY_MFMA], (1, 1): [GENERIC, GENERIC], (1, 0): [0]}
    for variant in (0, 1):
        a, b = (y.view(np.uint8) for y, _ in got[variant, 1])
        c = got[variant, 0][0][0].view(np.uint8)
        assert np.array_equal(a, b), variant
        assert np.array_equal(a, c), variant


def test_adjoint_inplace_two_components_halo(gpu):
    """one process, two components, the construction of test_mixed_two_components_halo: the image
    of a (4,2,2,2) lattice split in two along x, each component's domain the whole lattice.  The
    image pieces of A^H (A's domains) overlap and are summed; x carries the image labels and is
    split like the image, y like it too."""
    import torch
    import superbblas_amd as sb
    lat, bi, bd, ncols, dtype = (4, 2, 2, 2), 24, 24, 12, C128
    op = Op(lat, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, y0, ncols)
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
    dimx = [1] + list(lat) + list(split(bi)) + [ncols]
    hx = [1, 2] + dimx[2:]
    px = [([0, 2 * c, 0, 0, 0, 0, 0, 0], hx) for c in range(2)]
    n2 = x.size // 2
    vx = [torch.from_numpy(x[c * n2:(c + 1) * n2].copy()).to(gpu) for c in range(2)]
    vy = [torch.from_numpy(y0[c * n2:(c + 1) * n2].copy()).to(gpu) for c in range(2)]
    before = sb.tune_get("bsr.adj_copy_bytes")
    try:
        with tuned(adj_inplace=1):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", px, "pxyztscn", [0] * 8, dimx, dimx, vx, 0.0, px,
                          "pXYZTSCn", [0] * 8, dimx, dimx, "p", vy)
            torch.cuda.synchronize()
            used, held = sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.adj_copy_bytes")
    finally:
        h.destroy()
    assert used == MFMA and held == before, (used, held, before)
    assert np.array_equal(np.concatenate([v.cpu().numpy() for v in vy]), ref)


def test_adjoint_inplace_powers(gpu):
    """y[p] = (A^H)^(p+1) x for p = 0, 1 on a square 16x16 operator in complex<double>: the first
    power's pieces become the second one's x.  As in test_mixed_powers a component of A^H x is at
    most 5 * 16 * 2 * 36 = 5760 in size and one of the second power at most
    5 * 16 * 2 * 6 * 5760 < 2^23: exact, far below 2^50."""
    import torch
    import superbblas_amd as sb
    b, ncols, dtype = 16, 12, C128
    op = Op(LAT, b, b, dtype)
    x = int_valued(op.vol * b * ncols, dtype, 2)
    zero = np.zeros(op.vol * b * ncols, dtype)
    y1 = adjoint_reference(op, x, zero, ncols)
    y2 = adjoint_reference(op, y1, zero, ncols)
    assert max(np.abs(y2.real).max(), np.abs(y2.imag).max()) < 2.0 ** 50
    ox, dimx = layout(LAT, b, ncols, True, False)
    oy, _ = layout(LAT, b, ncols, True, True)
    dimy = [2] + dimx[1:]
    h = create(op, gpu)
    ty = torch.from_numpy(sentinel(2 * op.vol * b * ncols, dtype)).to(gpu)
    try:
        with tuned(adj_inplace=1):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx, dimx,
                          [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy,
                          "p", [ty])
            torch.cuda.synchronize()
            used = sb.tune_get("bsr.last_kernel")
    finally:
        h.destroy()
    assert used == MFMA, used
    assert np.array_equal(ty.cpu().numpy(), np.concatenate([y1, y2]))


def test_adjoint_inplace_x_through_a_temporary(gpu):
    """x ordered pxynztsc -- neither row nor column major -- is copied to a temporary"""
    import torch
    import superbblas_amd as sb
    bi = bd = 24
    ncols, dtype = 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bi * ncols, dtype, 2)
    y0 = sentinel(op.vol * bd * ncols, dtype)
    ref = adjoint_reference(op, x, y0, ncols)
    s, c = split(bi)
    xdev = np.ascontiguousarray(x.reshape(*LAT, s, c, ncols).transpose(0, 1, 6, 2, 3, 4, 5)).reshape(-1)
    dimx = [1, LAT[0], LAT[1], ncols, LAT[2], LAT[3], s, c]
    oy, dimy = layout(LAT, bd, ncols, True, True)
    h = create(op, gpu)
    ty = torch.from_numpy(y0.copy()).to(gpu)
    try:
        with tuned(adj_inplace=1):
            sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pxynztsc", [0] * 8, dimx, dimx,
                          [torch.from_numpy(xdev).to(gpu)], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy,
                          dimy, "p", [ty])
            torch.cuda.synchronize()
            used = sb.tune_get("bsr.last_kernel")
    finally:
        h.destroy()
    assert used == MFMA, used
    assert np.array_equal(ty.cpu().numpy(), ref)


@pytest.mark.parametrize("spin,color,kernel", [(4, 3, 15), (2, 3, 16)])
def test_adjoint_inplace_leaves_kronecker_operators(gpu, spin, color, kernel):
    """operators of create_kron_bsr ignore the key: their adjoint is in place already"""
    import superbblas_amd as sb
    from _kron_adjoint import adjoint_ref, int_vector, lattice_case
    from test_gpu_kron_adjoint import apply_adjoint, make_op
    L, ncols = 2, 3
    ii, jj, vals, kron, A = lattice_case(L, color, color, spin, spin)
    V = L ** 4
    x = int_vector(V * color * ncols * spin)
    ref = adjoint_ref(A, x, V, color, color, spin, spin, ncols)
    before = sb.tune_get("bsr.adj_copy_bytes")
    op, _, _ = make_op(sb, gpu, L, color, color, spin, spin, False, ii, jj, vals, kron)
    try:
        with tuned(adj_inplace=1):
            used, out = apply_adjoint(sb, gpu, op, L, color, color, spin, spin, ncols, x)
            held = sb.tune_get("bsr.adj_copy_bytes")
    finally:
        op.destroy()
    assert used == kernel and held == before, (used, held, before)
    assert np.array_equal(out, ref)


@functools.lru_cache(maxsize=None)
def forward_case(spin, color, ncols):
    from test_gpu_bsr import lattice_operator
    L = 4
    dim, ii, jj, vals, nb = lattice_operator(L, spin, color)
    b, vol = spin * color, L ** 4
    x = int_valued(vol * b * ncols, C128, 2)
    ref = np.zeros(vol * b * ncols, C128)
    oracle_bsr(TYPE_OF[np.dtype(C128)], dim, 0, vol, b, b, ii, jj, vals, False, x, ncols, True, ref,
               ncols, True, ncols, 1.0)
    return dim, ii, jj, vals, x, ref


@pytest.mark.parametrize("spin,color,ncols,forms", [(4, 3, 3, (7, 8)), (1, 3, 2, (1, 2, 3))])
def test_adjoint_inplace_leaves_forward_products(gpu, spin, color, ncols, forms):
    """A x with the key at 1 runs the kernels it runs today (12x12 and 3x3 operators; dense
    blocks below)"""
    import torch
    import superbblas_amd as sb
    L = 4
    dim, ii, jj, vals, x, ref = forward_case(spin, color, ncols)
    full = [([0] * 6, dim)]
    blk = [1, 1, 1, 1, spin, color]
    h = sb.create_bsr(full, dim, full, dim, blk, blk, False, [torch.from_numpy(ii).to(gpu)],
                      [torch.from_numpy(jj).to(gpu)], [torch.from_numpy(vals).to(gpu)])
    dimx = [1, L, L, L, L, spin, color, ncols]
    ty = torch.zeros(ref.size, dtype=torch.complex128, device=gpu)
    used = {}
    try:
        for key in (0, 1):
            with tuned(adj_inplace=key):
                sb.bsr_krylov(1.0, h, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx,
                              dimx, [torch.from_numpy(x).to(gpu)], 0.0, [([0] * 8, dimx)], "pxyztscn",
                              [0] * 8, dimx, dimx, "p", [ty])
                torch.cuda.synchronize()
                used[key] = sb.tune_get("bsr.last_kernel")
                assert np.array_equal(ty.cpu().numpy(), ref), key
    finally:
        h.destroy()
    assert used[0] in forms and used[1] == used[0], used


def test_adjoint_inplace_leaves_forward_dense_blocks(gpu):
    """A x of a 48x48 operator with the key at 1: form 14, also after an A^H product in place"""
    import superbblas_amd as sb
    from test_gpu_bsr_blocks import reference
    bi, bd, ncols, dtype = 48, 48, 12, C64
    op = Op(LAT, bi, bd, dtype)
    x = int_valued(op.vol * bd * ncols, dtype, 2)
    y0 = sentinel(op.vol * bi * ncols, dtype)
    ref = reference(op, x, y0, ncols)
    before = sb.tune_get("bsr.adj_copy_bytes")
    h = create(op, gpu)
    try:
        with tuned(adj_inplace=1):
            ya, fa = apply(gpu, op, h, x, y0, ncols)
            _, fh = apply(gpu, op, h, x, y0, ncols, adjoint=True)
            yb, fb = apply(gpu, op, h, x, y0, ncols)
            held = sb.tune_get("bsr.adj_copy_bytes")
    finally:
        h.destroy()
    assert (fa, fh, fb) == (COPY_MFMA, MFMA, COPY_MFMA) and held == before
    assert np.array_equal(ya, ref) and np.array_equal(yb, ref)
