#!/usr/bin/env python3
"""Config-2 GEMM (16^4, n = 64, complex<double>): the lean main loop ("gemm.lean") against the
generic loader-wave kernel (not part of the product).  LEAN: the values of the key to time,
interleaved over ROUNDS rounds in one warm process (empty: the key is not touched, for a build
without it); every timing is the library's HIP-event time of the GEMM kernel over REPS calls, a
round's figure the median of TIMINGS timings.  SB_ROOT: import the package from another tree (an
A/B against another build of the library).  Results of all values must be bit-identical."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    leans = [int(v) for v in os.environ.get("LEAN", "0,1").split(",") if v != ""] or [None]
    rounds, reps = int(os.environ.get("ROUNDS", "1")), int(os.environ.get("REPS", "10"))
    timings = int(os.environ.get("TIMINGS", "5"))
    tag = os.environ.get("TAG", "")
    L, n = 16, 64
    d0 = [L, n, 4, L, L, L, 3]
    dr = [L, n, 4, n, 4]
    vol0 = 1
    for x in d0:
        vol0 *= x
    g = torch.Generator(device=dev).manual_seed(5)
    v0 = torch.randn(vol0, dtype=torch.complex128, device=dev, generator=g)
    v1 = torch.randn(vol0, dtype=torch.complex128, device=dev, generator=g)
    vr = torch.zeros(L * n * 4 * n * 4, dtype=torch.complex128, device=dev)
    z7, z5 = [0] * 7, [0] * 5

    def step():
        sb.contraction(1.0, [(z7, d0)], z7, d0, d0, "tnsxyzc", False, [v0], [(z7, d0)], z7, d0,
                       d0, "tNSxyzc", False, [v1], 0.0, [(z5, dr)], z5, dr, dr, "tNSns", [vr])

    for _ in range(int(os.environ.get("WARM", "100"))):  # clocks up
        step()
    torch.cuda.synchronize()
    ref = None
    for rnd in range(rounds):
        for lean in leans:
            last = None
            if lean is not None:
                sb.tune_set("gemm.lean", lean)
            step()
            torch.cuda.synchronize()
            if lean is not None:
                last = sb.tune_get("gemm.last_lean")
            ts = []
            sb.tune_set("gemm.clock", 1)
            for _ in range(timings):
                sb.timings_enable(True)
                sb.timings_filter("gemm")
                sb.timings_reset()
                for _ in range(reps):
                    step()
                torch.cuda.synchronize()
                ms, calls = sb.timings_get("gemm")
                sb.timings_enable(False)
                ts.append(ms / calls)
            cyc, ticks = sb.tune_get("gemm.clock_cycles"), sb.tune_get("gemm.clock_ticks")
            sb.tune_set("gemm.clock", 0)
            if ref is None:
                ref = vr.clone()
            same = bool(torch.equal(ref, vr))
            ts.sort()
            print(json.dumps({"tag": tag, "round": rnd, "lean": lean, "last_lean": last,
                              "gemm_ms_median": round(ts[len(ts) // 2], 5),
                              "gemm_ms_min": round(ts[0], 5), "gemm_ms_max": round(ts[-1], 5),
                              "shader_clock_GHz": round(cyc / (ticks * 10.0), 4) if ticks else None,
                              "bits_equal_first": same}), flush=True)
    if leans[0] is not None:
        sb.tune_set("gemm.lean", 1)


if __name__ == "__main__":
    main()
