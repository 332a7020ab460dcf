"""Lean main loop of the complex<double> 128x128x16 K-major LDS-DMA GEMM (sbx_tune_set "gemm.lean",
on by default; gemm_lean_kernel): launches of whole 128 x 128 tiles and whole 16-deep slabs
without split groups take a kernel with the arithmetic of the generic one and none of its
per-piece bookkeeping.

What is pinned, all complex128 with K-major operands:
 * the read-back "gemm.last_lean": 1 for an eligible launch, 0 with gemm.lean 0 and for every
   ineligible launch (m = 130, k = 40, gemm.dma_nt 1, an operand with split groups), which still
   matches the oracle;
 * gemm.lean 1 gives exactly the bits of gemm.lean 0 -- 1, 2, 3 and 13 slabs per split (the
   prologue slab, the buffer flip, the last slab), several splits of 1-3 slabs, one tile, 2 x 2
   tiles and 1 x 2 tiles, batch 1 and 3, the four conjugation combinations, alpha = 1 / beta = 0
   and complex alpha and beta on a random C, with and without split-K (the split-K cases also
   cover the lean kernel's partial stores staged through LDS: the workspace, and so the sums of
   splitk_reduce_kernel, must hold the generic kernel's bits);
 * the oracle (the tolerance of tests/test_gpu_gemm.py);
 * two calls in a row give the same bits."""
import functools

import numpy as np
import pytest

from _common import oracle_contraction, oracle_gemm, random_valued, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10  # complex128 in the table of tests/test_gpu_gemm.py
CD = np.complex128
KEYS = ("gemm.lean", "gemm.splits", "gemm.dma_nt")
ALPHA, BETA = 0.5 - 0.5j, 0.25 + 1j


@functools.lru_cache(maxsize=None)
def _data(m, n, k, batch):
    a = random_valued(k * m * batch, CD, 51)
    b = random_valued(k * n * batch, CD, 52)
    c0 = random_valued(m * n * batch, CD, 53)
    for v in (a, b, c0):
        v.setflags(write=False)
    return a, b, c0


@functools.lru_cache(maxsize=None)
def _oracle(ta, m, n, k, batch):
    """op(A) B by the oracle (alpha = 1, beta = 0), computed once per case and left unchanged"""
    a, b, _ = _data(m, n, k, batch)
    ref = np.zeros(m * n * batch, CD)
    oracle_gemm(ta, "N", m, n, k, 1.0, a, k, k * m, b, k, k * n, 0.0, ref, m, m * n, batch)
    ref.setflags(write=False)
    return ref


def _gemm(gpu, ta, m, n, k, batch, alpha=1.0, beta=0.0):
    """C = alpha op(A) B + beta C0 on the GPU, (ta, 'N') on K-major buffers; (C, last_lean)"""
    import torch
    import superbblas_amd as sb
    a, b, c0 = _data(m, n, k, batch)
    t_a, t_b = torch.from_numpy(a.copy()).to(gpu), torch.from_numpy(b.copy()).to(gpu)
    t_c = torch.from_numpy(c0.copy()).to(gpu)
    sb.xgemm_batch_strided(ta, "N", m, n, k, alpha, t_a, k, k * m, t_b, k, k * n, beta, t_c, m,
                           m * n, batch)
    torch.cuda.synchronize()
    return t_c.cpu().numpy(), sb.tune_get("gemm.last_lean")


class _tunes:
    def __init__(self, **kv):
        self.kv = {"gemm." + k: v for k, v in kv.items()}

    def __enter__(self):
        import superbblas_amd as sb
        self.old = {key: sb.tune_get(key) for key in KEYS}
        for key, v in self.kv.items():
            sb.tune_set(key, v)

    def __exit__(self, *exc):
        import superbblas_amd as sb
        for key, v in self.old.items():
            sb.tune_set(key, v)


def _case(gpu, ta, m, n, k, batch, splits=0, expect=1, **tunes):
    """lean 1 against lean 0 (bits), the read-backs, the oracle, a repeated call"""
    with _tunes(lean=0, splits=splits, **tunes):
        g0, l0 = _gemm(gpu, ta, m, n, k, batch)
        g0s, _ = _gemm(gpu, ta, m, n, k, batch, ALPHA, BETA)
    with _tunes(lean=1, splits=splits, **tunes):
        g1, l1 = _gemm(gpu, ta, m, n, k, batch)
        g1b, _ = _gemm(gpu, ta, m, n, k, batch)
        g1s, l1s = _gemm(gpu, ta, m, n, k, batch, ALPHA, BETA)
    print("last_lean: lean 0 %d, lean 1 %d" % (l0, l1))
    assert l0 == 0
    assert l1 == expect and l1s == expect
    assert np.array_equal(g1, g0), "gemm.lean 1 differs from gemm.lean 0"
    assert np.array_equal(g1s, g0s), "gemm.lean 1 differs from gemm.lean 0 (alpha, beta)"
    assert np.array_equal(g1b, g1), "two calls differ"
    ref = _oracle(ta, m, n, k, batch)
    _, _, c0 = _data(m, n, k, batch)
    e1, e2 = rel_err(g1, ref), rel_err(g1s, ALPHA * ref + BETA * c0)
    print("rel err vs the oracle: %.3g (alpha 1, beta 0), %.3g (alpha, beta)" % (e1, e2))
    assert e1 < TOL
    assert e2 < TOL


@pytest.mark.parametrize("m,n,k,batch", [(128, 128, 16, 1), (128, 128, 32, 3), (128, 256, 48, 3),
                                         (256, 256, 208, 1), (256, 256, 48, 3)])
@pytest.mark.parametrize("ta", ["T", "C"])
def test_lean_one_split(gpu, ta, m, n, k, batch):
    """1, 2, 3 and 13 slabs in one split (k < 256: the library does not split); one tile, 1 x 2
    and 2 x 2 tiles, batch 1 and 3 (the tile index and its XCD remap)"""
    _case(gpu, ta, m, n, k, batch)


@pytest.mark.parametrize("m,n,k,batch,splits", [(128, 128, 112, 1, 3), (256, 256, 80, 3, 3),
                                                (128, 256, 48, 1, 3), (128, 128, 512, 1, 0),
                                                (256, 128, 592, 3, 5)])
@pytest.mark.parametrize("ta", ["T", "C"])
def test_lean_split_k(gpu, ta, m, n, k, batch, splits):
    """the split-K workspace path: splits of 3 + 3 + 1, 2 + 2 + 1 and 1 + 1 + 1 slabs
    (gemm.splits 3), the library's own 2 splits of 16 slabs at k = 512, 5 splits of 8 + ... + 5"""
    _case(gpu, ta, m, n, k, batch, splits)


@pytest.mark.parametrize("m,n,k,batch,tunes", [(130, 128, 48, 1, {}), (128, 130, 48, 2, {}),
                                               (128, 128, 40, 2, {}),
                                               (128, 128, 48, 2, {"dma_nt": 1})])
def test_lean_fallbacks(gpu, m, n, k, batch, tunes):
    """a ragged last tile, a k that is no slab multiple and the non-temporal DMA policy stay on
    the generic kernel (read-back 0) and match the oracle"""
    _case(gpu, "C", m, n, k, batch, expect=0, **tunes)


@functools.lru_cache(maxsize=None)
def _lattice(o0, d0, o1, d1, seed):
    v0 = random_valued(int(np.prod(d0)), CD, seed)
    v1 = random_valued(int(np.prod(d1)), CD, seed + 1)
    c0 = random_valued(2 * 128 * 128, CD, seed + 2)
    for v in (v0, v1, c0):
        v.setflags(write=False)
    return v0, v1, c0


def _contract(gpu, o0, d0, conj0, o1, d1, conj1, alpha, beta, seed):
    """"tba" = alpha o0 o1 + beta C0 through sb.contraction (t = 2, a = b = 128) on the GPU and by
    the oracle; (C, last_lean, oracle)"""
    import torch
    import superbblas_amd as sb
    d0, d1, dr = list(d0), list(d1), [2, 128, 128]
    v0, v1, c0 = _lattice(o0, tuple(d0), o1, tuple(d1), seed)
    z0, z1, zr = [0] * len(d0), [0] * len(d1), [0] * 3
    ref = c0.copy()
    oracle_contraction(alpha, o0, z0, d0, d0, conj0, v0, o1, z1, d1, d1, conj1, v1, beta, "tba",
                       zr, dr, dr, ref)
    t0, t1 = torch.from_numpy(v0.copy()).to(gpu), torch.from_numpy(v1.copy()).to(gpu)
    tr = torch.from_numpy(c0.copy()).to(gpu)
    sb.contraction(alpha, [(z0, d0)], z0, d0, d0, o0, conj0, [t0], [(z1, d1)], z1, d1, d1, o1,
                   conj1, [t1], beta, [(zr, dr)], zr, dr, dr, "tba", [tr])
    torch.cuda.synchronize()
    return tr.cpu().numpy(), sb.tune_get("gemm.last_lean"), ref


@pytest.mark.parametrize("conj0", [False, True])
@pytest.mark.parametrize("conj1", [False, True])
@pytest.mark.parametrize("splits", [0, 2])
def test_lean_conjugations(gpu, conj0, conj1, splits):
    """the four conjugation combinations (the MFMA sign modifiers of the lean kernel against the
    generic kernel's sign flips), 3 slabs in one split and 2 + 1 in two, complex alpha and beta"""
    args = ("tak", (2, 128, 48), conj0, "tbk", (2, 128, 48), conj1, ALPHA, BETA, 61)
    with _tunes(lean=0, splits=splits):
        g0, l0, ref = _contract(gpu, *args)
    with _tunes(lean=1, splits=splits):
        g1, l1, _ = _contract(gpu, *args)
    assert (l0, l1) == (0, 1)
    assert np.array_equal(g1, g0), "gemm.lean 1 differs from gemm.lean 0"
    err = rel_err(g1, ref)
    print("rel err vs the oracle: %.3g" % err)
    assert err < TOL


def test_lean_split_groups_fall_back(gpu):
    """a summed group of two runs of memory (x and k of "txak"): k = 2 x 24 = 48 is a slab
    multiple, but the operands' k index is a split group: the generic kernel"""
    args = ("txak", (2, 2, 128, 24), True, "txbk", (2, 2, 128, 24), False, 1.0, 0.0, 71)
    with _tunes(lean=1):
        g1, l1, ref = _contract(gpu, *args)
    assert l1 == 0
    err = rel_err(g1, ref)
    print("rel err vs the oracle: %.3g" % err)
    assert err < TOL
