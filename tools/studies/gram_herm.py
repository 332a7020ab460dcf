#!/usr/bin/env python3
"""A Gram matrix A^H A through xgemm_batch_strided with one buffer as both operands ('C', 'N' on a
K-major buffer; default m = n = 256, k = 49 152, batch 1, complex<double>: M, K, BATCH, DTYPE) with
the Hermitian-output mode off and on (HERM=0,1: "gemm.herm"; the upper triangle of tiles only, 3 of
4 at two tiles per side), the settings interleaved ROUNDS times in one process; REPS calls per
timing after WARM calls; results compared with torch.  SB_ROOT: import the package from another
tree (an A/B against another build of the library, whose keys it may lack).  Not part of the
product."""
import json
import os
import sys

import torch

sys.path.insert(0, os.environ.get("SB_ROOT") or
                os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import superbblas_amd as sb  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    m, k, batch = (int(os.environ.get(v, d)) for v, d in (("M", 256), ("K", 49152), ("BATCH", 1)))
    dtype = getattr(torch, os.environ.get("DTYPE", "complex128"))
    herms = [int(v) for v in os.environ.get("HERM", "0,1").split(",")]
    reps, warm = int(os.environ.get("REPS", "100")), int(os.environ.get("WARM", "20"))
    a = torch.randn(batch * m * k, dtype=dtype, device=dev)
    c = torch.empty(batch * m * m, dtype=dtype, device=dev)
    av = a.view(batch, m, k)  # column-major k x m per batch entry
    ref = torch.einsum("bik,bjk->bji", av.conj(), av).reshape(-1)
    fl = (8.0 if dtype.is_complex else 2.0) * batch * m * m * k
    for r in range(int(os.environ.get("ROUNDS", "5"))):
        for herm in herms:
            try:
                sb.tune_set("gemm.herm", herm)
            except sb.SuperbblasError:  # (a build without the key: the full product only)
                if herm:
                    raise

            def f():
                sb.xgemm_batch_strided("C", "N", m, m, k, 1.0, a, k, k * m, a, k, k * m, 0.0, c,
                                       m, m * m, batch)
            for _ in range(warm):
                f()
            torch.cuda.synchronize()
            err = (torch.linalg.vector_norm(c - ref) / torch.linalg.vector_norm(ref)).item()
            try:
                last = sb.tune_get("gemm.last_herm")
            except sb.SuperbblasError:
                last = None
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                f()
            e.record()
            torch.cuda.synchronize()
            t = s.elapsed_time(e) / reps / 1e3
            print(json.dumps({"round": r, "m": m, "k": k, "batch": batch, "dtype": str(dtype),
                              "herm": herm, "last_herm": last, "ms": round(t * 1e3, 4),
                              "TFLOPs_full_product": round(fl / t / 1e12, 2),
                              "rel_err_vs_einsum": err}), flush=True)
    try:
        sb.tune_set("gemm.herm", 0)
    except sb.SuperbblasError:
        pass


if __name__ == "__main__":
    main()
