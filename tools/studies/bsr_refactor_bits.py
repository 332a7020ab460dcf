#!/usr/bin/env python3
"""Bit-identity study (not part of the product): the BSR kernels of two builds on random data.
The exact tests use small integers, which any summation order gets right; this one writes y of a
periodic 9-point stencil operator on a 3^4 lattice with random values, for every combination of
  blocks   (16,16), (20,36), (48,48), (128,128)
  columns  1, 17, 40
  types    float, double, complex<float>, complex<double>, and float / complex<float> operators on
           double / complex<double> vectors
  product  A x, and A^H x with "bsr.adj_inplace" 1 (x with the image labels)
  form     "bsr.blk_mfma" 2 (the dense-block kernel: forms 14 / 16 / 17; the mixed adjoint 18) and
           0 (the generic kernel: forms 0 / 18)
in a worker process per build (two libraries cannot share a process), then compares the bytes:

  SB_ROOT=<other tree> python3 tools/studies/bsr_refactor_bits.py --worker /tmp/a &&
  python3 tools/studies/bsr_refactor_bits.py --worker /tmp/b &&
  python3 tools/studies/bsr_refactor_bits.py --compare /tmp/a /tmp/b

A worker writes PREFIX.bin (every y, one after the other) and PREFIX.json (one record per case:
the case, "bsr.last_kernel" and the offset and size of its y); it takes seconds.  --compare
prints the cases that differ and the count, exit status 1 if any does."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BLOCKS = [(16, 16), (20, 36), (48, 48), (128, 128)]
COLS = [1, 17, 40]
# (operator type, vector type)
TYPES = [("float32", "float32"), ("float64", "float64"), ("complex64", "complex64"),
         ("complex128", "complex128"), ("float32", "float64"), ("complex64", "complex128")]
L = 3


def worker(prefix):
    import numpy as np
    import torch
    sys.path.insert(0, os.environ.get("SB_ROOT") or ROOT)
    import superbblas_amd as sb

    dev = torch.device("cuda:0")
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
    tjj = torch.from_numpy(jj.reshape(-1)).to(dev)
    tii = torch.from_numpy(np.full(V, 9, np.int32)).to(dev)

    def random(n, dtype, seed):
        rng = np.random.default_rng(seed)
        dtype = np.dtype(dtype)
        if dtype.kind == "c":
            real = np.float32 if dtype == np.complex64 else np.float64
            return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype), real
        return rng.standard_normal(n).astype(dtype), dtype

    records = []
    with open(prefix + ".bin", "wb") as out:
        for bi, bd in BLOCKS:
            dimi, dimd = [L, L, L, L, 2, bi // 2], [L, L, L, L, 2, bd // 2]
            for tv, tx in TYPES:
                vals = torch.from_numpy(random(V * 9 * bi * bd, tv, 1)[0]).to(dev)
                op = sb.create_bsr([([0] * 6, dimi)], dimi, [([0] * 6, dimd)], dimd, [1, 1, 1, 1, 2, bi // 2],
                                   [1, 1, 1, 1, 2, bd // 2], False, [tii], [tjj], [vals])
                for adjoint in (0, 1):
                    sb.tune_set("bsr.adj_inplace", adjoint)
                    bx, by = (bi, bd) if adjoint else (bd, bi)
                    for n in COLS:
                        dimx = [1, L, L, L, L, 2, bx // 2, n]
                        dimy = [1, L, L, L, L, 2, by // 2, n]
                        ox, oy = ("pxyztscn", "pXYZTSCn") if adjoint else ("pXYZTSCn", "pxyztscn")
                        x = torch.from_numpy(random(V * bx * n, tx, 2)[0]).to(dev)
                        for blk_mfma in (2, 0):
                            sb.tune_set("bsr.blk_mfma", blk_mfma)
                            y = torch.zeros(V * by * n, dtype=x.dtype, device=dev)
                            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], ox, [0] * 8, dimx,
                                          dimx, [x], 0.0, [([0] * 8, dimy)], oy, [0] * 8, dimy, dimy, "p", [y])
                            torch.cuda.synchronize()
                            data = y.cpu().numpy().tobytes()
                            records.append({"block": [bi, bd], "types": [tv, tx], "adjoint": adjoint, "n": n,
                                            "blk_mfma": blk_mfma, "last_kernel": sb.tune_get("bsr.last_kernel"),
                                            "offset": out.tell(), "bytes": len(data)})
                            out.write(data)
                sb.tune_set("bsr.adj_inplace", 0)
                sb.tune_set("bsr.blk_mfma", 1)
                op.destroy()
    with open(prefix + ".json", "w") as f:
        json.dump(records, f)
    print("%d cases, %d bytes of y -> %s.bin" % (len(records), records[-1]["offset"] + records[-1]["bytes"], prefix))


def compare(pa, pb):
    ra, rb = json.load(open(pa + ".json")), json.load(open(pb + ".json"))
    if len(ra) != len(rb):
        sys.exit("the two runs hold %d and %d cases" % (len(ra), len(rb)))
    differ, forms = 0, {}
    with open(pa + ".bin", "rb") as fa, open(pb + ".bin", "rb") as fb:
        for a, b in zip(ra, rb):
            case = {k: a[k] for k in ("block", "types", "adjoint", "n", "blk_mfma")}
            if case != {k: b[k] for k in case}:
                sys.exit("the two runs' cases differ: %s / %s" % (a, b))
            fa.seek(a["offset"])
            fb.seek(b["offset"])
            same = (a["bytes"] == b["bytes"] and a["last_kernel"] == b["last_kernel"] and
                    fa.read(a["bytes"]) == fb.read(b["bytes"]))
            forms[a["last_kernel"]] = forms.get(a["last_kernel"], 0) + 1
            if not same:
                differ += 1
                print("differs: %s (forms %d / %d)" % (json.dumps(case), a["last_kernel"], b["last_kernel"]))
    print("%d cases (by form of the first run: %s), %d differ" %
          (len(ra), ", ".join("%d: %d" % kv for kv in sorted(forms.items())), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
