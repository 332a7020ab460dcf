#!/usr/bin/env python3
"""Mixed-precision BSR study (not part of the product): the multigrid coarse operators -- a
periodic 9-point stencil on an 8^4 lattice with square blocks of BLOCKS (16, 24, 32, 48, 64), N
right-hand sides (1, 4, 12, 16, 32, 64), x pXYZTSCn (row major) -> y pxyztscn, random values --
kept in complex<float> and applied to complex<double> vectors, against the same operator in one
type.  Four forms per point, alternating over ROUNDS rounds (at least 3, after one warm-up round)
in one warm process; every figure is the library's HIP-event time of the "bsr" kernels over REPS
calls:
  a  mixed, matrix cores: complex<float> operator, complex<double> vectors, "bsr.mixed" 1 with
     "bsr.blk_mfma" 2 (bsr_blk_mfma_kernel's mixed form at any column count)
  b  mixed, generic: "bsr.mixed" 0
  c  the same values as a complex<double> operator, complex<double> vectors, default dispatch
     (what a caller has to do without the mixed product)
  d  all in complex<float>, default dispatch (the traffic floor)
FORMS selects among them (default abcd).  SB_ROOT: import the package from another tree (an A/B
against another build of the library: FORMS=cd for a build without the mixed product).  One JSON
line per point: the median of the rounds and their spread (max - min) per form, the algorithmic
bytes -- 8 (9 b^2 V) + 16 (2 b V n) + 4 (9 V + V + 1) for the mixed forms, es (9 b^2 V + 2 b V n) +
4 (9 V + V + 1) for c and d -- and their fraction of 8 TB/s."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

# form: (operator in double, vectors in double, {tune key: value})
FORMS = {"a": (False, True, {"bsr.mixed": 1, "bsr.blk_mfma": 2}),
         "b": (False, True, {"bsr.mixed": 0}),
         "c": (True, True, {}),
         "d": (False, False, {})}


def stencil(L):
    V = L ** 4
    sites = np.array(np.unravel_index(np.arange(V), (L, L, L, L))).T
    jj = np.zeros((V, 9, 6), np.int32)
    jj[:, 0, :4] = sites
    k = 1
    for d in range(4):
        for s in (-1, 1):
            c = sites.copy()
            c[:, d] = (c[:, d] + s) % L
            jj[:, k, :4] = c
            k += 1
    return jj


def main():
    dev = torch.device("cuda:0")
    forms = [f for f in os.environ.get("FORMS", "abcd") if f in FORMS]
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "3"))), int(os.environ.get("REPS", "5"))
    blocks = [int(v) for v in os.environ.get("BLOCKS", "16,24,32,48,64").split(",")]
    ns = [int(v) for v in os.environ.get("N", "1,4,12,16,32,64").split(",")]
    tag = os.environ.get("TAG", "")
    L = 8
    V = L ** 4
    jj = torch.from_numpy(stencil(L).reshape(-1)).to(dev)
    ii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for b in blocks:
        spin, color = 2, b // 2
        dim = [L, L, L, L, spin, color]
        full = [([0] * 6, dim)]
        blk = [1, 1, 1, 1, spin, color]
        vals = {False: torch.randn(V * 9 * b * b, dtype=torch.complex64, device=dev, generator=g)}
        if any(FORMS[f][0] for f in forms):
            vals[True] = vals[False].to(torch.complex128)
        ops = {w: sb.create_bsr(full, dim, full, dim, blk, blk, False, [ii], [jj], [v])
               for w, v in vals.items()}
        for n in ns:
            dimx = [1, L, L, L, L, spin, color, n]
            px = [([0] * 8, dimx)]
            xs = {True: torch.randn(V * b * n, dtype=torch.complex128, device=dev, generator=g)}
            xs[False] = xs[True].to(torch.complex64)
            ys = {w: torch.empty_like(x) for w, x in xs.items()}

            def f(fm):
                wide_op, wide_vec, _ = FORMS[fm]
                sb.bsr_krylov(1.0, ops[wide_op], "xyztsc", "XYZTSC", px, "pXYZTSCn", [0] * 8, dimx,
                              dimx, [xs[wide_vec]], 0.0, px, "pxyztscn", [0] * 8, dimx, dimx, "p",
                              [ys[wide_vec]])
            us = {fm: [] for fm in forms}
            last = {}
            for rnd in range(rounds + 1):  # round 0: the warm-up
                for fm in forms:
                    keys = FORMS[fm][2]
                    old = {k: sb.tune_get(k) for k in keys}
                    for k, v in keys.items():
                        sb.tune_set(k, v)
                    f(fm)
                    torch.cuda.synchronize()
                    last[fm] = sb.tune_get("bsr.last_kernel")
                    sb.timings_enable(True)
                    sb.timings_reset()
                    for _ in range(reps):
                        f(fm)
                    torch.cuda.synchronize()
                    ms, calls = sb.timings_get("bsr")
                    sb.timings_enable(False)
                    for k, v in old.items():
                        sb.tune_set(k, v)
                    if rnd > 0:
                        us[fm].append(ms / calls * 1e3)
            rec = {"tag": tag, "block": b, "n": n}
            for fm in forms:
                wide_op, wide_vec, _ = FORMS[fm]
                by = ((16 if wide_op else 8) * 9.0 * b * b * V + (16 if wide_vec else 8) * 2.0 * b * V * n +
                      4.0 * (9 * V + V + 1))
                t = sorted(us[fm])
                med = t[len(t) // 2]
                rec[fm] = {"last_kernel": last[fm], "us": round(med, 1), "spread_us": round(t[-1] - t[0], 1),
                           "bytes": by, "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
            print(json.dumps(rec), flush=True)
        for op in ops.values():
            op.destroy()
        del vals, ops


if __name__ == "__main__":
    main()
