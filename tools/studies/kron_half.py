#!/usr/bin/env python3
"""Half-precision Kronecker study (not part of the product): the lattice's fine operator as
create_kron_bsr keeps it -- a periodic 9-point stencil of 3x3 colour blocks times one 4x4 spin
matrix per direction (1, 1 -+ gamma_mu) on the lattices LATS (16^4 and 16^3 x 64), N right-hand
sides (1, 4, 8, 12, 16, 32, 64), x pXYZTCnS -> y pxyztcns (A x) or the labels swapped (A^H x),
random colour values in [-1, 1] rounded to binary16 -- kept in complex32 under complex<float>
vectors ("bsr.kron_half" 1) against the same values widened to complex<float> on the same-type
path.  The forms of a point alternate over ROUNDS rounds (5, after one warm-up round) in one warm
process; every figure is the library's HIP-event time of the "bsr" kernels over REPS calls:
  x  A x, complex32 operator (bsr_kron_lds_kernel<f16x2, float2> from 4 columns,
     bsr_kron_kernel<f16x2, float2> below)
  s  A x, the same values widened to complex<float>: what a caller does without the half
     operator -- code this change leaves as it was, the yardstick
  a  A^H x, complex32 operator (bsr_kron_adj_kernel<f16x2, float2, ...>)
  h  A^H x, the widened operator
FORMS selects among them (default xsah).  One JSON line per point: the median of the rounds and
their spread (max - min) per form, the algorithmic bytes -- ev (81 V + 144) + 8 (2 12 V n) +
4 (9 V) with ev the bytes of a value (4 or 8) --, their fraction of 8 TB/s, and the ratios s / x
(above 1: the half operator is faster than the all-single one) and h / a of the medians, each with
the lowest and highest ratio of the single rounds beside it."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

from kron_mixed import stencil, wilson_spin  # noqa: E402

# form: (operator in complex32, adjoint)
FORMS = {"x": (True, False), "s": (False, False), "a": (True, True), "h": (False, True)}
SPIN, COLOR = 4, 3


def main():
    dev = torch.device("cuda:0")
    forms = [f for f in os.environ.get("FORMS", "xsah") if f in FORMS]
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "5"))), int(os.environ.get("REPS", "5"))
    lats = [tuple(int(v) for v in lat.split("x"))
            for lat in os.environ.get("LATS", "16x16x16x16,16x16x16x64").split(",")]
    ns = [int(v) for v in os.environ.get("N", "1,4,8,12,16,32,64").split(",")]
    tag = os.environ.get("TAG", "")
    g = torch.Generator(device=dev).manual_seed(7)
    sb.tune_set("bsr.kron_half", 1)
    for lat in lats:
        V = int(np.prod(lat))
        jj = torch.from_numpy(stencil(lat).reshape(-1)).to(dev)
        ii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)
        dim = list(lat) + [SPIN, COLOR]
        full = [([0] * 6, dim)]
        blk, kr = [1, 1, 1, 1, 1, COLOR], [1, 1, 1, 1, SPIN, 1]
        # binary16 values, and the same values widened (exactly) to float
        r16 = (torch.rand(V * 81 * 2, dtype=torch.float32, device=dev, generator=g) * 2 - 1).to(torch.float16)
        k16 = torch.view_as_real(torch.from_numpy(wilson_spin()).to(dev)).reshape(-1).to(torch.float16)
        vals = {True: (torch.view_as_complex(r16.view(-1, 2)), torch.view_as_complex(k16.view(-1, 2))),
                False: (torch.view_as_complex(r16.to(torch.float32).view(-1, 2)),
                        torch.view_as_complex(k16.to(torch.float32).view(-1, 2)))}
        ops = {w: sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False, [ii], [jj], [v], [k])
               for w, (v, k) in vals.items() if any(FORMS[f][0] == w for f in forms)}
        for n in ns:
            dimx = [1] + list(lat) + [COLOR, n, SPIN]
            px = [([0] * 8, dimx)]
            x = torch.randn(V * 12 * n, dtype=torch.complex64, device=dev, generator=g)
            y = torch.empty_like(x)

            def f(fm):
                ox, oy = ("pxyztcns", "pXYZTCnS") if FORMS[fm][1] else ("pXYZTCnS", "pxyztcns")
                sb.bsr_krylov(1.0, ops[FORMS[fm][0]], "xyztsc", "XYZTSC", px, ox, [0] * 8, dimx, dimx, [x],
                              0.0, px, oy, [0] * 8, dimx, dimx, "p", [y])
            us = {fm: [] for fm in forms}
            last, outs = {}, {}
            for rnd in range(rounds + 1):  # round 0: the warm-up
                for fm in forms:
                    f(fm)
                    torch.cuda.synchronize()
                    last[fm] = (sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed"))
                    if rnd == 0:
                        outs[fm] = y.clone()
                    sb.timings_enable(True)
                    sb.timings_reset()
                    for _ in range(reps):
                        f(fm)
                    torch.cuda.synchronize()
                    ms, calls = sb.timings_get("bsr")
                    sb.timings_enable(False)
                    if rnd > 0:
                        us[fm].append(ms / calls * 1e3)
            rec = {"tag": tag, "lat": "x".join(str(v) for v in lat), "n": n}
            for fm in forms:
                ev = 4 if FORMS[fm][0] else 8
                by = ev * (81.0 * V + 144) + 8 * 2.0 * 12 * V * n + 4.0 * 9 * V
                t = sorted(us[fm])
                med = t[len(t) // 2]
                rec[fm] = {"last_kernel": last[fm][0], "last_mixed": last[fm][1], "us": round(med, 1),
                           "spread_us": round(t[-1] - t[0], 1), "bytes": by,
                           "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
            for num, den in (("s", "x"), ("h", "a")):
                if num in rec and den in rec:
                    per = [a / b for a, b in zip(us[num], us[den])]
                    rec[num + "_over_" + den] = round(rec[num]["us"] / rec[den]["us"], 3)
                    rec[num + "_over_" + den + "_rounds"] = [round(min(per), 3), round(max(per), 3)]
                    # (both operators hold the same values: the same product, up to the sums' order)
                    rec[num + "_vs_" + den + "_equal"] = bool(torch.equal(outs[num], outs[den]))
            print(json.dumps(rec), flush=True)
            del x, y, outs
        for op in ops.values():
            op.destroy()
        del vals, ops, r16
    sb.tune_set("bsr.kron_half", 0)


if __name__ == "__main__":
    main()
