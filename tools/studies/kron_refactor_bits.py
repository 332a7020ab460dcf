#!/usr/bin/env python3
"""Bit-identity study (not part of the product): the Kronecker BSR kernels of two builds on random
data, in the manner of bsr_refactor_bits.py.  The exact tests use small integers, which any
summation order gets right; this one writes y of the periodic 9-point stencil operator (3x3 colour
blocks, 4x4 spin matrices) on 3^4 and 4^4 lattices with random values, for
  columns  1, 4, 8, 12, 16, 17, 40
  types    complex<double>, complex<float>, and complex<float> / float operators under
           complex<double> / double vectors ("bsr.kron_mixed" 1)
  forward  the matrix-core kernels at every column count ("bsr.kron_mfma_min_cols" 1), packed slots
           on and off, x staged 0-3 neighbours ahead, y per lane or through the ring (forms 5, 6);
           "bsr.kron_mfma" 0: the LDS VALU kernel from 4 columns, the 3x3 x 4x4 kernel below;
           2x2 spin matrices: the generic kernel
  spin     "bsr.kron_spin" 1 and 2 with the Wilson spin matrices (complex<double>, from 8 columns)
  adjoint  "bsr.kron_adj" 1 (staged from 32 columns), 2 (never staged), 0 (the generic kernel)
in a worker process per build (two libraries cannot share a process), then compares the bytes:

  SB_ROOT=<other tree> timeout -k 10 240 python3 tools/studies/kron_refactor_bits.py --worker /tmp/a &&
  timeout -k 10 240 python3 tools/studies/kron_refactor_bits.py --worker /tmp/b &&
  python3 tools/studies/kron_refactor_bits.py --compare /tmp/a /tmp/b

A worker writes PREFIX.bin and PREFIX.json (one record per case: the case, "bsr.last_kernel" and
the offset and size of its y); --compare is bsr_refactor_bits.py's: it prints the cases that
differ and the count, exit status 1 if any does."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COLS = [1, 4, 8, 12, 16, 17, 40]
# (operator type, vector type)
TYPES = [("complex128", "complex128"), ("complex64", "complex64"), ("complex64", "complex128"),
         ("float32", "float64")]
KEYS = ("bsr.kron_mfma", "bsr.kron_mfma_min_cols", "bsr.kron_pack", "bsr.kron_xlds", "bsr.kron_ylds",
        "bsr.kron_spin", "bsr.kron_adj")
DEFAULT = (1, 8, 1, 1, 0, 0, 1)


def wilson_spin():
    import numpy as np
    i_ = 1j
    g = [np.array([[0, 0, 0, i_], [0, 0, i_, 0], [0, -i_, 0, 0], [-i_, 0, 0, 0]]),
         np.array([[0, 0, 0, -1], [0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]]),
         np.array([[0, 0, i_, 0], [0, 0, 0, -i_], [-i_, 0, 0, 0], [0, i_, 0, 0]]),
         np.array([[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]])]
    ks = [np.eye(4)]
    for gm in g:
        ks += [np.eye(4) - gm, np.eye(4) + gm]
    return np.array(ks, np.complex128).ravel()


def variants(tv, tx, spin, n):
    """(name, adjoint, values of KEYS) of a (types, spin size, columns) point"""
    out = []
    if spin == 2:
        return [("generic", 0, DEFAULT), ("adj_generic", 1, DEFAULT)]
    if tx == "complex128":
        for pack in (1, 0):
            for xl in (0, 1, 2, 3):
                for yl in ((0, 1) if xl else (0,)):
                    out.append(("mfma", 0, (1, 1, pack, xl, yl, 0, 1)))
    out.append(("valu", 0, (0, 8, 1, 1, 0, 0, 1)))
    if tv == tx == "complex128" and n >= 8:
        out += [("spin1", 0, (1, 8, 1, 1, 0, 1, 1)), ("spin2", 0, (1, 8, 1, 1, 0, 2, 1))]
    out += [("adj", 1, DEFAULT), ("adj_unstaged", 1, (1, 8, 1, 1, 0, 0, 2)), ("adj_generic", 1, (1, 8, 1, 1, 0, 0, 0))]
    return out


def worker(prefix):
    import numpy as np
    import torch
    sys.path.insert(0, os.environ.get("SB_ROOT") or ROOT)
    import superbblas_amd as sb

    dev = torch.device("cuda:0")
    sb.tune_set("bsr.kron_mixed", 1)

    def random(n, dtype, seed):
        rng = np.random.default_rng(seed)
        dtype = np.dtype(dtype)
        if dtype.kind == "c":
            return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)
        return rng.standard_normal(n).astype(dtype)

    records = []
    with open(prefix + ".bin", "wb") as out:
        for L in (3, 4):
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
            for tv, tx in TYPES:
                for spin, kind in ((4, "random"), (4, "wilson"), (2, "random")):
                    if kind == "wilson" and not tv == tx == "complex128":
                        continue
                    vals = torch.from_numpy(random(V * 81, tv, 1)).to(dev)
                    kron = wilson_spin().astype(tv) if kind == "wilson" else random(9 * spin * spin, tv, 3)
                    dim = [L, L, L, L, spin, 3]
                    full = [([0] * 6, dim)]
                    op = sb.create_kron_bsr(full, dim, full, dim, [1, 1, 1, 1, 1, 3], [1, 1, 1, 1, 1, 3],
                                            [1, 1, 1, 1, spin, 1], [1, 1, 1, 1, spin, 1], False, [tii], [tjj],
                                            [vals], [torch.from_numpy(kron).to(dev)])
                    for n in COLS:
                        dimx = [1, L, L, L, L, 3, n, spin]
                        px = [([0] * 8, dimx)]
                        x = torch.from_numpy(random(V * 3 * n * spin, tx, 2)).to(dev)
                        for name, adjoint, values in variants(tv, tx, spin, n):
                            if (kind == "wilson") != name.startswith("spin"):
                                continue
                            for key, v in zip(KEYS, values):
                                sb.tune_set(key, v)
                            ox, oy = ("pxyztcns", "pXYZTCnS") if adjoint else ("pXYZTCnS", "pxyztcns")
                            y = torch.zeros_like(x)
                            sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", px, ox, [0] * 8, dimx, dimx, [x], 0.0, px,
                                          oy, [0] * 8, dimx, dimx, "p", [y])
                            torch.cuda.synchronize()
                            data = y.cpu().numpy().tobytes()
                            records.append({"L": L, "types": [tv, tx], "spin": spin, "kron": kind, "n": n,
                                            "variant": name, "keys": list(values),
                                            "last_kernel": sb.tune_get("bsr.last_kernel"),
                                            "offset": out.tell(), "bytes": len(data)})
                            out.write(data)
                    for key, v in zip(KEYS, DEFAULT):
                        sb.tune_set(key, v)
                    op.destroy()
    sb.tune_set("bsr.kron_mixed", 0)
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
            case = {k: a[k] for k in ("L", "types", "spin", "kron", "n", "variant", "keys")}
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
