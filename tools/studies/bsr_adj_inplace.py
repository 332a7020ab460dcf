#!/usr/bin/env python3
"""In-place adjoint study (not part of the product): y = A^H x (x with the image labels) of
periodic 9-point stencil operators on an 8^4 lattice -- square blocks of BLOCKS (16, 24, 48, 64
and the 3x3 and 12x12 lattice operators), complex<float> and complex<double> (TYPES), N right-hand
sides (1, 4, 12, 16), x pxyztscn (row major) -> y pXYZTSCn, random values -- two ways:
  inplace  "bsr.adj_inplace" 1 in this tree: A's value array read through the entry list
           ("bsr.last_kernel" 17 / 18)
  copy     A^H through the conjugated, regrouped copy, in the library of the tree BASE (the build
           of the commit before the in-place adjoint: the baseline is not the code under study;
           BASE unset: this tree with the key at 0; BASE_KEY=1: BASE's library with the key at 1
           too, its in-place kernels against this tree's, the "copy" columns then hold BASE's)
Each way runs in a worker process of its own (two libraries cannot share a process); the driver
hands out the rounds in turn, so the rounds of the two ways alternate, both processes warm:
ROUNDS rounds (at least 3) after one warm-up round, every figure the library's HIP-event time of
the "bsr" kernels over REPS calls.  One JSON line per point -- the median of the rounds and their
spread (max - min) per way -- then the table; per operator the bytes of its values and of the
copy ("bsr.adj_copy_bytes" after a product with the key at 0; 0 while only in-place products ran)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def env_list(name, default):
    return [v for v in os.environ.get(name, default).split(",") if v]


def points():
    for b in (int(v) for v in env_list("BLOCKS", "16,24,48,64,3,12")):
        for t in env_list("TYPES", "complex64,complex128"):
            yield b, t


def worker(inplace):
    import numpy as np
    import torch
    sys.path.insert(0, os.environ.get("SB_ROOT") or ROOT)
    import superbblas_amd as sb

    dev = torch.device("cuda:0")
    rounds, reps = max(3, int(os.environ.get("ROUNDS", "3"))), int(os.environ.get("REPS", "5"))
    ns = [int(v) for v in env_list("N", "1,4,12,16")]
    L = 8
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
    g = torch.Generator(device=dev).manual_seed(7)
    if inplace:
        sb.tune_set("bsr.adj_inplace", 1)
    for b, tname in points():
        dt = getattr(torch, tname)
        spin, color = {3: (1, 3), 12: (4, 3)}.get(b, (2, b // 2))
        dim = [L, L, L, L, spin, color]
        full = [([0] * 6, dim)]
        blk = [1, 1, 1, 1, spin, color]
        vals = torch.randn(V * 9 * b * b, dtype=dt, device=dev, generator=g)
        op = sb.create_bsr(full, dim, full, dim, blk, blk, False, [tii], [tjj], [vals])
        for n in ns:
            dimx = [1, L, L, L, L, spin, color, n]
            px = [([0] * 8, dimx)]
            x = torch.randn(V * b * n, dtype=dt, device=dev, generator=g)
            y = torch.empty_like(x)

            def f():
                sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", px, "pxyztscn", [0] * 8, dimx, dimx, [x], 0.0,
                              px, "pXYZTSCn", [0] * 8, dimx, dimx, "p", [y])
            for rnd in range(rounds + 1):  # round 0: the warm-up
                if not sys.stdin.readline():
                    return
                f()
                torch.cuda.synchronize()
                last = sb.tune_get("bsr.last_kernel")
                sb.timings_enable(True)
                sb.timings_reset()
                for _ in range(reps):
                    f()
                torch.cuda.synchronize()
                ms, calls = sb.timings_get("bsr")
                sb.timings_enable(False)
                print(json.dumps({"block": b, "type": tname, "n": n, "round": rnd, "last_kernel": last,
                                  "us": ms / calls * 1e3}), flush=True)
            del x, y
        # the operator's bytes: its values, and the copy a product with the key at 0 adds
        if not sys.stdin.readline():
            return
        rec = {"block": b, "type": tname, "values_bytes": vals.numel() * vals.element_size()}
        try:
            rec["copy_bytes_now"] = sb.tune_get("bsr.adj_copy_bytes")
            if inplace:
                sb.tune_set("bsr.adj_inplace", 0)
                dimx = [1, L, L, L, L, spin, color, 1]
                x = torch.randn(V * b, dtype=dt, device=dev, generator=g)
                y = torch.empty_like(x)
                sb.bsr_krylov(1.0, op, "xyztsc", "XYZTSC", [([0] * 8, dimx)], "pxyztscn", [0] * 8, dimx,
                              dimx, [x], 0.0, [([0] * 8, dimx)], "pXYZTSCn", [0] * 8, dimx, dimx, "p", [y])
                torch.cuda.synchronize()
                rec["copy_bytes_after_key0"] = sb.tune_get("bsr.adj_copy_bytes")
                sb.tune_set("bsr.adj_inplace", 1)
        except sb.SuperbblasError:  # a library from before the key
            pass
        print(json.dumps(rec), flush=True)
        op.destroy()
        del vals, op


def driver():
    rounds = max(3, int(os.environ.get("ROUNDS", "3")))
    ns = [int(v) for v in env_list("N", "1,4,12,16")]
    base = os.environ.get("BASE")
    # BASE_KEY 1: BASE reads in place too (this tree's in-place kernels against another build's)
    ways = {"inplace": ("1", ROOT), "copy": (os.environ.get("BASE_KEY", "0"), base or ROOT)}
    procs = {}
    for way, (flag, root) in ways.items():
        env = dict(os.environ, SB_ROOT=root)
        procs[way] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", flag],
                                      stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(way):
        p = procs[way]
        p.stdin.write("go\n")
        p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            raise RuntimeError("the %s worker ended (exit %s)" % (way, p.wait()))
        return json.loads(line)

    rows, mem = [], []
    try:
        for b, tname in points():
            for n in ns:
                us = {w: [] for w in ways}
                last = {}
                for rnd in range(rounds + 1):
                    for w in ways:
                        r = ask(w)
                        assert (r["block"], r["type"], r["n"], r["round"]) == (b, tname, n, rnd), r
                        last[w] = r["last_kernel"]
                        if rnd > 0:
                            us[w].append(r["us"])
                rec = {"block": b, "type": tname, "n": n}
                for w in ways:
                    t = sorted(us[w])
                    rec[w] = {"last_kernel": last[w], "us": round(t[len(t) // 2], 1),
                              "spread_us": round(t[-1] - t[0], 1)}
                rec["inplace_over_copy"] = round(rec["inplace"]["us"] / rec["copy"]["us"], 3)
                print(json.dumps(rec), flush=True)
                rows.append(rec)
            m = {w: ask(w) for w in ways}
            mem.append(m["inplace"])
            print(json.dumps({"memory": m}), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait()
    print()
    print("A^H x, 8^4 9-point operators; us = median of %d rounds (spread = max - min); copy: %s" %
          (rounds, "the library of BASE" if base else "this tree, key 0"))
    print("%5s %-10s %3s | %-18s | %-18s | %s" % ("block", "type", "n", "in place: form us (spread)",
                                                 "copy: form us (spread)", "in place / copy"))
    for r in rows:
        i, c = r["inplace"], r["copy"]
        print("%5d %-10s %3d | %4d %9.1f (%6.1f) | %4d %9.1f (%6.1f) | %6.3f" %
              (r["block"], r["type"], r["n"], i["last_kernel"], i["us"], i["spread_us"], c["last_kernel"],
               c["us"], c["spread_us"], r["inplace_over_copy"]))
    print()
    print("device bytes of the operator's values: in place (no copy) / with the copy of the key at 0")
    for m in mem:
        if "copy_bytes_after_key0" in m:
            print("%5d %-10s %13d + %d = %13d / + %13d = %13d" %
                  (m["block"], m["type"], m["values_bytes"], m["copy_bytes_now"],
                   m["values_bytes"] + m["copy_bytes_now"], m["copy_bytes_after_key0"] - m["copy_bytes_now"],
                   m["values_bytes"] + m["copy_bytes_after_key0"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--worker":
        worker(sys.argv[2] == "1")
    else:
        driver()
