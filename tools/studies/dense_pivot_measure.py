#!/usr/bin/env python3
"""The error ratios behind F in tests/test_gpu_dense_pivot.py: runs that file on the GPU and
prints, per operation, kernel path and element type, the worst ratio of the kernel's error to
max(e_lapack, n eps) over the rand_capped cases (e_lapack: numpy's LAPACK in the same precision
on the same matrix, both against the long-double truth), and the F the rule gives: the next
power of two at or above twice the worst ratio.  The ratios are recorded before each test
asserts, so the run measures whatever F the file holds.

`dense_pivot_measure.py tail` (no GPU): how the per-matrix ratio of two small errors spreads.  A
float64 emulation of the Gauss-Jordan kernel's order (reciprocal pivot, no FMA) and numpy's
LAPACK on 4000 rand_capped matrices per size, each against the long-double truth: quantiles of
emulation / max(LAPACK, n eps), of LAPACK / max(emulation, n eps), and both errors' largest
multiple of eps cond_2.  Not part of the product."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tail():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _dense import ld_inverse, rand_capped
    eps = np.finfo(np.float64).eps

    def rel(x, t):
        return (np.abs(x - t).max(axis=(1, 2)) / np.abs(t).max(axis=(1, 2))).astype(np.float64)

    def gauss_jordan(a):
        nt, n = a.shape[:2]
        m = np.concatenate([a, np.broadcast_to(np.eye(n), a.shape)], 2)
        bi = np.arange(nt)
        for j in range(n):
            p = j + np.argmax(np.abs(m[:, j:, j]), 1)
            rj, rp = m[bi, j].copy(), m[bi, p].copy()
            m[bi, p] = rj
            m[bi, j] = rp * (1 / rp[:, j:j + 1])
            f = m[:, :, j:j + 1].copy()
            f[:, j] = 0
            m -= f * m[:, j:j + 1, :]
        return m[:, :, n:]

    print("%3s %28s %28s %12s" % ("n", "emulation / LAPACK", "LAPACK / emulation", "err/(eps cond)"))
    print("%3s %6s %6s %7s %6s %6s %6s %7s %6s %6s %6s" % (
        "", "median", "99%", "99.9%", "max", "median", "99%", "99.9%", "max", "emul.", "LAPACK"))
    for n in (2, 5, 12, 16):
        a = rand_capped(4000, n, np.float64, seed=78)
        truth, cond = ld_inverse(a), np.linalg.cond(a)
        el, eg = rel(np.linalg.inv(a), truth), rel(gauss_jordan(a), truth)
        r, q = eg / np.maximum(el, n * eps), el / np.maximum(eg, n * eps)
        print("%3d %6.2f %6.2f %7.2f %6.2f %6.2f %6.2f %7.2f %6.2f %6.3f %6.3f" % (
            n, np.median(r), np.quantile(r, .99), np.quantile(r, .999), r.max(), np.median(q),
            np.quantile(q, .99), np.quantile(q, .999), q.max(), (eg / eps / cond).max(),
            (el / eps / cond).max()))
    return 0


def main():
    if sys.argv[1:2] == ["tail"]:
        return tail()
    rc = pytest.main([os.path.join(ROOT, "tests", "test_gpu_dense_pivot.py"), "-m", "gpu", "-q",
                      "-p", "no:cacheprovider", "--durations=5"] + sys.argv[1:])
    ratios = sys.modules["test_gpu_dense_pivot"].RATIOS
    worst = {}
    for op, path, t, n, r, err, lap, cond in ratios:
        key = (op, path.split(" ")[0], t)
        if key not in worst or r > worst[key][0]:
            worst[key] = (r, err, lap, cond, err / cond, n, path)
    print("\nworst ratio per operation, kernel path and type, with that matrix's error, numpy's "
          "error (both in eps of the type), cond_2 and error / (eps cond)")
    print("%-10s %-10s %-11s %8s %9s %9s %8s %9s  at" % (
        "operation", "path", "type", "ratio", "err/eps", "numpy/eps", "cond", "err/epsc"))
    for key in sorted(worst):
        print("%-10s %-10s %-11s %8.3f %9.2f %9.2f %8.1f %9.3f  n=%d %s" % (key + worst[key]))
    for op, t in sorted({k[::2] for k in worst}):
        w = max(v[0] for k, v in worst.items() if k[::2] == (op, t))
        print("%s %s: worst ratio %.3f of %d cases -> F = %d" % (
            op, t, w, sum(1 for x in ratios if (x[0], x[2]) == (op, t)),
            2 ** math.ceil(math.log2(2 * w))))
    print("pytest exit code %d" % rc)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
