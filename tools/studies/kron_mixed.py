#!/usr/bin/env python3
"""Mixed-precision Kronecker study (not part of the product): the lattice's fine operator as
create_kron_bsr keeps it -- a periodic 9-point stencil of 3x3 colour blocks times one 4x4 spin
matrix per direction (1, 1 -+ gamma_mu) on the lattices LATS (16^4 and 16^3 x 64), N right-hand
sides (1, 4, 8, 12, 16, 32, 64), x pXYZTCnS -> y pxyztcns (A x) or the labels swapped (A^H x),
random values -- kept in complex<float> under complex<double> vectors ("bsr.kron_mixed" 1).
The forms of a point alternate over ROUNDS rounds (5, after one warm-up round) in one warm
process; every figure is the library's HIP-event time of the "bsr" kernels over REPS calls:
  m  A x, complex<float> operator, the matrix-core kernels at every column count
     ("bsr.kron_mfma_min_cols" 1: bsr_kron_mfma_packed_kernel below 16 columns where the column
     count divides 16 W, bsr_kron_mfma_kernel otherwise)
  v  A x, complex<float> operator, the VALU kernels ("bsr.kron_mfma" 0: bsr_kron_lds_kernel from 4
     columns, bsr_kron_kernel below)
  x  A x, complex<float> operator, the default dispatch
  d  A x, the same values widened to complex<double>, the default dispatch: what a caller does
     without the mixed product -- code this change leaves as it was, the yardstick
  a  A^H x, complex<float> operator, the default dispatch (bsr_kron_adj_kernel)
  h  A^H x, the widened operator, the default dispatch
FORMS selects among them (default mvxdah); XLDS, if set, is "bsr.kron_xlds" for the whole run (the
matrix-core kernels' instantiations with x staged that many neighbours ahead).  One JSON line per point: the median of the rounds and
their spread (max - min) per form, the algorithmic bytes -- ev (81 V + 144) + 16 (2 12 V n) +
4 (9 V) with ev the bytes of a value (8 or 16) --, their fraction of 8 TB/s, and the ratios
v / m (above 1: the matrix-core form is the faster mixed form), d / x (above 1: the mixed product
is faster than the all-double one) and h / a of the medians."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

# form: (operator in complex<float>, adjoint, {tune key: value})
FORMS = {"m": (True, False, {"bsr.kron_mfma": 1, "bsr.kron_mfma_min_cols": 1}),
         "v": (True, False, {"bsr.kron_mfma": 0}),
         "x": (True, False, {}),
         "d": (False, False, {}),
         "a": (True, True, {}),
         "h": (False, True, {})}
SPIN, COLOR = 4, 3


def stencil(lat):
    V = int(np.prod(lat))
    sites = np.array(np.unravel_index(np.arange(V), lat)).T
    jj = np.zeros((V, 9, 6), np.int32)
    jj[:, 0, :4] = sites
    k = 1
    for d in range(4):
        for s in (-1, 1):
            c = sites.copy()
            c[:, d] = (c[:, d] + s) % lat[d]
            jj[:, k, :4] = c
            k += 1
    return jj


def wilson_spin():
    """1, 1 -+ gamma_mu (chiral basis), as bench.py's Wilson operator"""
    i_ = 1j
    g = [np.array([[0, 0, 0, i_], [0, 0, i_, 0], [0, -i_, 0, 0], [-i_, 0, 0, 0]]),
         np.array([[0, 0, 0, -1], [0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]]),
         np.array([[0, 0, i_, 0], [0, 0, 0, -i_], [-i_, 0, 0, 0], [0, i_, 0, 0]]),
         np.array([[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]])]
    ks = [np.eye(4)]
    for gm in g:
        ks += [np.eye(4) - gm, np.eye(4) + gm]
    return np.array(ks, np.complex64).ravel()


def main():
    dev = torch.device("cuda:0")
    forms = [f for f in os.environ.get("FORMS", "mvxdah") if f in FORMS]
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "5"))), int(os.environ.get("REPS", "5"))
    lats = [tuple(int(v) for v in lat.split("x"))
            for lat in os.environ.get("LATS", "16x16x16x16,16x16x16x64").split(",")]
    ns = [int(v) for v in os.environ.get("N", "1,4,8,12,16,32,64").split(",")]
    tag = os.environ.get("TAG", "")
    g = torch.Generator(device=dev).manual_seed(7)
    sb.tune_set("bsr.kron_mixed", 1)
    if os.environ.get("XLDS"):
        sb.tune_set("bsr.kron_xlds", int(os.environ["XLDS"]))
    for lat in lats:
        V = int(np.prod(lat))
        jj = torch.from_numpy(stencil(lat).reshape(-1)).to(dev)
        ii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)
        dim = list(lat) + [SPIN, COLOR]
        full = [([0] * 6, dim)]
        blk, kr = [1, 1, 1, 1, 1, COLOR], [1, 1, 1, 1, SPIN, 1]
        r32 = torch.randn(V * 81 * 2, dtype=torch.float32, device=dev, generator=g)
        k32 = torch.from_numpy(wilson_spin()).to(dev)
        vals = {True: (torch.view_as_complex(r32.view(-1, 2)), k32),
                False: (torch.view_as_complex(r32.to(torch.float64).view(-1, 2)), k32.to(torch.complex128))}
        ops = {w: sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False, [ii], [jj], [v], [k])
               for w, (v, k) in vals.items() if any(FORMS[f][0] == w for f in forms)}
        for n in ns:
            dimx = [1] + list(lat) + [COLOR, n, SPIN]
            px = [([0] * 8, dimx)]
            x = torch.randn(V * 12 * n, dtype=torch.complex128, device=dev, generator=g)
            y = torch.empty_like(x)

            def f(fm):
                ox, oy = ("pxyztcns", "pXYZTCnS") if FORMS[fm][1] else ("pXYZTCnS", "pxyztcns")
                sb.bsr_krylov(1.0, ops[FORMS[fm][0]], "xyztsc", "XYZTSC", px, ox, [0] * 8, dimx, dimx, [x],
                              0.0, px, oy, [0] * 8, dimx, dimx, "p", [y])
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
                    last[fm] = (sb.tune_get("bsr.last_kernel"), sb.tune_get("bsr.last_mixed"))
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
            rec = {"tag": tag, "lat": "x".join(str(v) for v in lat), "n": n}
            for fm in forms:
                ev = 8 if FORMS[fm][0] else 16
                by = ev * (81.0 * V + 144) + 16 * 2.0 * 12 * V * n + 4.0 * 9 * V
                t = sorted(us[fm])
                med = t[len(t) // 2]
                rec[fm] = {"last_kernel": last[fm][0], "last_mixed": last[fm][1], "us": round(med, 1),
                           "spread_us": round(t[-1] - t[0], 1), "bytes": by,
                           "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
            for num, den in (("v", "m"), ("d", "x"), ("h", "a")):
                if num in rec and den in rec:
                    rec[num + "_over_" + den] = round(rec[num]["us"] / rec[den]["us"], 3)
            print(json.dumps(rec), flush=True)
            del x, y
        for op in ops.values():
            op.destroy()
        del vals, ops, r32
    sb.tune_set("bsr.kron_mixed", 0)


if __name__ == "__main__":
    main()
