#!/usr/bin/env python3
"""Half-precision BSR study (not part of the product): the multigrid coarse operators -- a
periodic 9-point stencil on an 8^4 lattice with square blocks of BLOCKS (16, 24, 32, 48, 64), N
right-hand sides (1, 4, 12, 16, 32, 64), x pXYZTSCn (row major) -> y pxyztscn, random values --
kept in complex32 (two IEEE binary16: re, im) and applied to complex<float> vectors, against the
same values as a complex<float> operator.  Three forms per point, alternating over ROUNDS rounds
(at least 3, after one warm-up round) in one warm process; every figure is the library's
HIP-event time of the "bsr" kernels over REPS calls:
  a  half operator, matrix cores: "bsr.mixed" 1 with "bsr.blk_mfma" 2 (bsr_blk_mfma_kernel's mixed
     form at any column count)
  b  half operator, generic: "bsr.mixed" 0
  d  the same values (widened) as a complex<float> operator, complex<float> vectors, default
     dispatch: what a caller does without the half product -- code this change leaves as it was,
     the yardstick
FORMS selects among them (default abd).  One JSON line per point: the median of the rounds and
their spread (max - min) per form, the algorithmic bytes -- 4 (9 b^2 V) + 8 (2 b V n) +
4 (10 V + 1) for a and b, 8 (9 b^2 V + 2 b V n) + 4 (10 V + 1) for d -- their fraction of 8 TB/s,
and the ratios d / a and b / a of the medians."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

# form: (operator in half, {tune key: value})
FORMS = {"a": (True, {"bsr.mixed": 1, "bsr.blk_mfma": 2}),
         "b": (True, {"bsr.mixed": 0}),
         "d": (False, {})}


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
    forms = [f for f in os.environ.get("FORMS", "abd") if f in FORMS]
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
        # (re, im) pairs rounded to binary16; the float operator holds the same values widened
        h16 = torch.randn(V * 9 * b * b * 2, dtype=torch.float32, device=dev, generator=g).to(torch.float16)
        vals = {True: torch.view_as_complex(h16.view(-1, 2)),
                False: torch.view_as_complex(h16.to(torch.float32).view(-1, 2))}
        ops = {w: sb.create_bsr(full, dim, full, dim, blk, blk, False, [ii], [jj], [v])
               for w, v in vals.items() if any(FORMS[f][0] == w for f in forms)}
        for n in ns:
            dimx = [1, L, L, L, L, spin, color, n]
            px = [([0] * 8, dimx)]
            x = torch.randn(V * b * n, dtype=torch.complex64, device=dev, generator=g)
            y = torch.empty_like(x)

            def f(fm):
                sb.bsr_krylov(1.0, ops[FORMS[fm][0]], "xyztsc", "XYZTSC", px, "pXYZTSCn", [0] * 8, dimx,
                              dimx, [x], 0.0, px, "pxyztscn", [0] * 8, dimx, dimx, "p", [y])
            us = {fm: [] for fm in forms}
            last = {}
            for rnd in range(rounds + 1):  # round 0: the warm-up
                for fm in forms:
                    keys = FORMS[fm][1]
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
                by = (4 if FORMS[fm][0] else 8) * 9.0 * b * b * V + 8 * 2.0 * b * V * n + 4.0 * (10 * V + 1)
                t = sorted(us[fm])
                med = t[len(t) // 2]
                rec[fm] = {"last_kernel": last[fm], "us": round(med, 1), "spread_us": round(t[-1] - t[0], 1),
                           "bytes": by, "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
            if "a" in rec:
                for fm in ("d", "b"):
                    if fm in rec:
                        rec[fm + "_over_a"] = round(rec[fm]["us"] / rec["a"]["us"], 3)
            print(json.dumps(rec), flush=True)
        for op in ops.values():
            op.destroy()
        del vals, ops, h16


if __name__ == "__main__":
    main()
