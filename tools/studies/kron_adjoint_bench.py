#!/usr/bin/env python3
"""Adjoint of the Kronecker operator (x with the image labels), microbenchmark (not part of the
product): the 16^4 Wilson-like operator of kron_bench.py (3x3 color blocks, sparse 4x4 spin
matrices 1 -/+ gamma_mu), kernel time from the library's HIP-event timers, warm, the forms
interleaved round by round, medians over the rounds.

  adj      y = A^H x, bsr_kron_adj_kernel (bsr.kron_adj 1)
  adj_gen  y = A^H x, bsr_kron_adj_generic_kernel (bsr.kron_adj 0)
  adj_ns   y = A^H x, bsr_kron_adj_kernel with the color blocks never staged in LDS (bsr.kron_adj 2;
           not in the default set of forms)
  fwd_valu y = A x of the same handle with bsr.kron_mfma 0 and bsr.kron_spin 0: the same loads and
           multiply-adds on the vector ALUs (the yardstick of the adjoint; runs on an older
           library too: FORMS=fwd_valu)
  fwd      y = A x at the defaults
  exp12    the route to A^H without this kernel: the operator expanded to 12x12 blocks
           (create_bsr) and contracted with the image side

FORMS=a,b,... selects forms, NS=1,4,... the column counts, DTYPES=complex128,... the types."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("SBX_PACKAGE_DIR") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kron_bench import lattice, wilson_spin_matrices  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (spec; about 6.3e12 achievable by a copy)


def main():
    dev = torch.device("cuda", 0)
    L = int(os.environ.get("L", "16"))
    forms = os.environ.get("FORMS", "adj,adj_gen,fwd_valu,fwd,exp12").split(",")
    ns = [int(v) for v in os.environ.get("NS", "1,4,12,16,64").split(",")]
    dtypes = os.environ.get("DTYPES", "complex128,complex64").split(",")
    rounds, reps = int(os.environ.get("ROUNDS", "7")), int(os.environ.get("REPS", "5"))
    spin, color = 4, 3
    V = L ** 4
    dim = [L, L, L, L, spin, color]
    full = [([0] * 6, dim)]
    ii, jj = lattice(L)
    tii, tjj = torch.from_numpy(ii).to(dev), torch.from_numpy(jj).to(dev)
    for dt in dtypes:
        dtype = getattr(torch, dt)
        torch.manual_seed(1)
        vals = torch.randn(V * 9 * color * color, dtype=dtype, device=dev)
        kron = torch.from_numpy(wilson_spin_matrices(False)).to(dtype).to(dev)
        blk, kr = [1, 1, 1, 1, 1, color], [1, 1, 1, 1, spin, 1]
        op = sb.create_kron_bsr(full, dim, full, dim, blk, blk, kr, kr, False, [tii], [tjj],
                                [vals], [kron])
        op12 = None
        if "exp12" in forms:
            # block k of the expanded operator: (a, i) x (b, d) = K_mu(a, b) U_k(i, d)
            v12 = torch.einsum("mab,vmid->vmaibd", kron.reshape(9, 4, 4),
                               vals.reshape(V, 9, 3, 3)).contiguous().reshape(-1)
            b12 = [1, 1, 1, 1, spin, color]
            op12 = sb.create_bsr(full, dim, full, dim, b12, b12, False, [tii], [tjj], [v12])
        es = vals.element_size()
        for n in ns:
            dimk = [1, L, L, L, L, color, n, spin]   # Kronecker layouts (site, color, n, spin)
            dim12 = [1, L, L, L, L, spin, color, n]  # plain layout (site, spin, color, n)
            x = torch.randn(V * 12 * n, dtype=dtype, device=dev)
            ys = {f: torch.zeros_like(x) for f in forms}
            pk, p12 = [([0] * 8, dimk)], [([0] * 8, dim12)]
            z8 = [0] * 8

            def call(form):
                if form in ("adj", "adj_gen", "adj_ns"):
                    sb.tune_set("bsr.kron_adj", {"adj": 1, "adj_gen": 0, "adj_ns": 2}[form])
                    sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", pk, "pxyztcns", z8, dimk, dimk, [x],
                                  0.0, pk, "pXYZTCnS", z8, dimk, dimk, "p", [ys[form]])
                elif form in ("fwd", "fwd_valu"):
                    sb.tune_set("bsr.kron_mfma", 1 if form == "fwd" else 0)
                    sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", pk, "pXYZTCnS", z8, dimk, dimk, [x],
                                  0.0, pk, "pxyztcns", z8, dimk, dimk, "p", [ys[form]])
                else:
                    sb.bsr_krylov(1.0, op12, "xyztsc", "XYZTSC", p12, "pxyztscn", z8, dim12, dim12,
                                  [x], 0.0, p12, "pXYZTSCn", z8, dim12, dim12, "p", [ys[form]])
                return sb.tune_get("bsr.last_kernel")

            sb.tune_set("bsr.kron_spin", 0)
            kernels, times = {}, {f: [] for f in forms}
            try:
                for f in forms:  # warm
                    for _ in range(3):
                        kernels[f] = call(f)
                torch.cuda.synchronize()
                if "adj" in forms and "adj_gen" in forms:
                    d = (ys["adj"] - ys["adj_gen"]).abs().max().item()
                    assert d <= 1e-4 * ys["adj_gen"].abs().max().item(), d
                sb.timings_enable(True)
                for _ in range(rounds):
                    for f in forms:
                        sb.timings_reset()
                        for _ in range(reps):
                            call(f)
                        torch.cuda.synchronize()
                        ms, calls = sb.timings_get("bsr")
                        times[f].append(ms / calls * 1e3)
                sb.timings_enable(False)
            finally:
                sb.tune_set("bsr.kron_mfma", 1)
                if "adj" in forms or "adj_gen" in forms or "adj_ns" in forms:
                    sb.tune_set("bsr.kron_adj", 1)
            for f in forms:
                us = statistics.median(times[f])
                # algorithmic bytes: the values, x and y once, the indices
                vbytes = es * (144 if f == "exp12" else 9) * 9 * V
                by = vbytes + es * 2 * 12 * V * n + 4.0 * 9 * V
                print(json.dumps({"dtype": dt, "n": n, "form": f, "kernel": kernels[f],
                                  "us": round(us, 1), "min_us": round(min(times[f]), 1),
                                  "max_us": round(max(times[f]), 1),
                                  "GBps": round(by / us / 1e3, 1),
                                  "hbm_peak_frac": round(by / (us * 1e-6) / HBM_PEAK, 3)}),
                      flush=True)
        op.destroy()
        if op12 is not None:
            op12.destroy()


if __name__ == "__main__":
    main()
