#!/usr/bin/env python3
"""12x12 mixed-precision BSR study (not part of the product): the lattice's fine operator -- a
periodic 9-point stencil with 12x12 (spin 4 x colour 3) blocks on the lattices LATS (16^4 and the
configs[4] chain's 16^3 x 64), N right-hand sides (1, 4, 12, 16, 32), x pXYZTSCn (row major) ->
y pxyztscn, random values -- kept one precision step below its vectors, for the PAIRS
  c32  complex32 values (two IEEE binary16: re, im), complex<float> vectors
  cf   complex<float> values, complex<double> vectors
The forms of a point alternate over ROUNDS rounds (5, after one warm-up round) in one warm
process; every figure is the library's HIP-event time of the "bsr" kernels over REPS calls:
  a  the 12x12 matrix-core kernels reading the narrow values: "bsr.mixed" 1 with
     "bsr.mixed12_min_cols" 1 (at any column count) and "bsr.mixed12_pack" 2 (the LDS-DMA form's
     ring slots packed at any column count)
  b  the generic mixed kernel: "bsr.mixed" 0
  d  the same values (widened) as an operator of the vectors' type, default dispatch: what a
     caller does without the mixed product -- code this change leaves as it was, the yardstick
  u  as a with "bsr.mixed12_pack" 0: the ring slots unpacked (each part rounded up to 1 KB)
  2, 3  as a with "bsr.blk_pd" 2 / 3 (that many blocks in flight ahead in the LDS-DMA form)
FORMS selects among them (default abd).  One JSON line per point: the median of the rounds and
their spread (max - min) per form, the algorithmic bytes -- ev (9 144 V) + ex (2 12 V n) +
4 (10 V + 1) with ev the bytes of a value (4 / 8 for a and b, 8 / 16 for d) and ex those of a
vector element (8 / 16) -- their fraction of 8 TB/s, and the ratios d / a and b / a of the
medians."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

# form: (operator in the narrow type, {tune key: value})
FORMS = {"a": (True, {"bsr.mixed": 1, "bsr.mixed12_min_cols": 1, "bsr.mixed12_pack": 2}),
         "u": (True, {"bsr.mixed": 1, "bsr.mixed12_min_cols": 1, "bsr.mixed12_pack": 0}),
         "2": (True, {"bsr.mixed": 1, "bsr.mixed12_min_cols": 1, "bsr.blk_pd": 2}),
         "3": (True, {"bsr.mixed": 1, "bsr.mixed12_min_cols": 1, "bsr.blk_pd": 3}),
         "b": (True, {"bsr.mixed": 0}),
         "d": (False, {})}
# pair: (bytes of a narrow value, bytes of a vector element, the vectors' torch type)
PAIRS = {"c32": (4, 8, torch.complex64), "cf": (8, 16, torch.complex128)}
SPIN, COLOR, B = 4, 3, 12


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


def main():
    dev = torch.device("cuda:0")
    forms = [f for f in os.environ.get("FORMS", "abd") if f in FORMS]
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "5"))), int(os.environ.get("REPS", "5"))
    lats = [tuple(int(v) for v in lat.split("x"))
            for lat in os.environ.get("LATS", "16x16x16x16,16x16x16x64").split(",")]
    pairs = [p for p in os.environ.get("PAIRS", "c32,cf").split(",") if p in PAIRS]
    ns = [int(v) for v in os.environ.get("N", "1,4,12,16,32").split(",")]
    tag = os.environ.get("TAG", "")
    g = torch.Generator(device=dev).manual_seed(7)
    for lat in lats:
        V = int(np.prod(lat))
        jj = torch.from_numpy(stencil(lat).reshape(-1)).to(dev)
        ii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)
        dim = list(lat) + [SPIN, COLOR]
        full = [([0] * 6, dim)]
        blk = [1, 1, 1, 1, SPIN, COLOR]
        for pair in pairs:
            ev, ex, xt = PAIRS[pair]
            # (re, im) pairs in the narrow type; the wide operator holds the same values widened
            r32 = torch.randn(V * 9 * B * B * 2, dtype=torch.float32, device=dev, generator=g)
            if pair == "c32":
                h16 = r32.to(torch.float16)
                vals = {True: torch.view_as_complex(h16.view(-1, 2)),
                        False: torch.view_as_complex(h16.to(torch.float32).view(-1, 2))}
            else:
                vals = {True: torch.view_as_complex(r32.view(-1, 2)),
                        False: torch.view_as_complex(r32.to(torch.float64).view(-1, 2))}
            del r32
            ops = {w: sb.create_bsr(full, dim, full, dim, blk, blk, False, [ii], [jj], [v])
                   for w, v in vals.items() if any(FORMS[f][0] == w for f in forms)}
            for n in ns:
                dimx = [1] + list(lat) + [SPIN, COLOR, n]
                px = [([0] * 8, dimx)]
                x = torch.randn(V * B * n, dtype=xt, device=dev, generator=g)
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
                rec = {"tag": tag, "lat": "x".join(str(v) for v in lat), "pair": pair, "n": n}
                for fm in forms:
                    by = (ev if FORMS[fm][0] else 2 * ev) * 9.0 * B * B * V + ex * 2.0 * B * V * n + 4.0 * (10 * V + 1)
                    t = sorted(us[fm])
                    med = t[len(t) // 2]
                    rec[fm] = {"last_kernel": last[fm], "us": round(med, 1), "spread_us": round(t[-1] - t[0], 1),
                               "bytes": by, "frac_hbm": round(by / (med * 1e-6) / 8e12, 4)}
                if "a" in rec:
                    for fm in ("d", "b", "u", "2", "3"):
                        if fm in rec:
                            rec[fm + "_over_a"] = round(rec[fm]["us"] / rec["a"]["us"], 3)
                print(json.dumps(rec), flush=True)
                del x, y
            for op in ops.values():
                op.destroy()
            del vals, ops


if __name__ == "__main__":
    main()
