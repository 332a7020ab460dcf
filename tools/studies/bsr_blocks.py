#!/usr/bin/env python3
"""Dense-block BSR study (not part of the product): the multigrid coarse operators -- a periodic
9-point stencil on an 8^4 lattice with square blocks of BLOCKS (16, 24, 32, 48, 64) of TYPES
(complex<float>, complex<double>), N right-hand sides (1, 4, 12, 16, 32, 64), x pXYZTSCn (row
major) -> y pxyztscn, random values -- on bsr_blk_mfma_kernel ("bsr.blk_mfma" 1) against the
generic kernel (0).  FORMS: the values of the key to time, alternating over ROUNDS rounds (at
least 3) in one warm process (empty: the key is not touched, for a build without it); every
figure is the library's HIP-event time of the "bsr" kernels over REPS calls.  SB_ROOT: import
the package from another tree (an A/B against another build of the library).  One JSON line per
point: the median of the rounds and their spread (max - min) per form, the algorithmic bytes
(bsr_bench.py's formula with the element size) and their fraction of 8 TB/s."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

TYPES = {"cfloat": (torch.complex64, 8), "cdouble": (torch.complex128, 16)}


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
    forms = [int(v) for v in os.environ.get("FORMS", "0,1").split(",") if v != ""] or [None]
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "3"))), int(os.environ.get("REPS", "5"))
    blocks = [int(v) for v in os.environ.get("BLOCKS", "16,24,32,48,64").split(",")]
    types = os.environ.get("TYPES", "cfloat,cdouble").split(",")
    ns = [int(v) for v in os.environ.get("N", "1,4,12,16,32,64").split(",")]
    tag = os.environ.get("TAG", "")
    L = 8
    V = L ** 4
    jj = torch.from_numpy(stencil(L).reshape(-1)).to(dev)
    ii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for tname in types:
        dt, es = TYPES[tname]
        for b in blocks:
            spin, color = 2, b // 2
            dim = [L, L, L, L, spin, color]
            vals = torch.randn(V * 9 * b * b, dtype=dt, device=dev, generator=g)
            full = [([0] * 6, dim)]
            blk = [1, 1, 1, 1, spin, color]
            op = sb.create_bsr(full, dim, full, dim, blk, blk, False, [ii], [jj], [vals])
            for n in ns:
                dimx = [1, L, L, L, L, spin, color, n]
                x = torch.randn(V * b * n, dtype=dt, device=dev, generator=g)
                y = torch.empty_like(x)
                px = [([0] * 8, dimx)]

                def f():
                    sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", px, "pXYZTSCn", [0] * 8, dimx, dimx,
                                  [x], 0.0, px, "pxyztscn", [0] * 8, dimx, dimx, "p", [y])
                us = {fm: [] for fm in forms}
                last = {}
                for rnd in range(rounds + 1):  # round 0: the warm-up
                    for fm in forms:
                        if fm is not None:
                            sb.tune_set("bsr.blk_mfma", fm)
                        f()
                        torch.cuda.synchronize()
                        last[fm] = sb.tune_get("bsr.last_kernel")
                        sb.timings_enable(True)
                        sb.timings_reset()
                        for _ in range(reps):
                            f()
                        torch.cuda.synchronize()
                        ms, calls = sb.timings_get("bsr")
                        sb.timings_enable(False)
                        if rnd > 0:
                            us[fm].append(ms / calls * 1e3)
                by = es * (9.0 * b * b * V + 2.0 * b * V * n) + 4.0 * (9 * V + V + 1)
                rec = {"tag": tag, "type": tname, "block": b, "n": n, "bytes": by}
                for fm in forms:
                    t = sorted(us[fm])
                    med = t[len(t) // 2]
                    key = "form%s" % ("" if fm is None else fm)
                    rec[key] = {"last_kernel": last[fm], "us": round(med, 1),
                                "spread_us": round(t[-1] - t[0], 1),
                                "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
                print(json.dumps(rec), flush=True)
            op.destroy()
            del vals
    if forms[0] is not None:
        sb.tune_set("bsr.blk_mfma", 1)


if __name__ == "__main__":
    main()
