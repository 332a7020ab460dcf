#!/usr/bin/env python3
"""Per-kernel summary of a device assembly file (hipcc ... --cuda-device-only -S).

  gemm_isa_summary.py FILE.s          one line per kernel symbol
  gemm_isa_summary.py OLD.s NEW.s     the kernels whose lines differ (exit status 1 if any)
  gemm_isa_summary.py OLD.s NEW.s RENAMES   the same, for kernels that changed their names: RENAMES
                                      holds lines "old_symbol new_symbol", and a kernel of OLD.s
                                      is compared with the kernel of NEW.s of its new name

A line holds the instruction count, the counts of MFMA, other vector-ALU, scalar, branch, LDS,
vector-memory and lane-move instructions (by opcode prefix alone) and the kernel descriptor's
next_free_vgpr / next_free_sgpr / private segment / group segment values: what "compiles to the
same instructions and register counts" means for a restructuring of kernels_gemm.hip.
"""
import collections
import re
import sys

CLASSES = [  # first matching prefix wins
    ("mfma", ("v_mfma", "v_smfmac")),
    ("lane", ("v_readlane", "v_readfirstlane", "v_writelane", "v_permlane", "ds_bpermute",
              "ds_permute", "ds_swizzle", "v_mov_b32_dpp")),
    ("valu", ("v_",)),
    ("branch", ("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")),
    ("salu", ("s_",)),
    ("lds", ("ds_",)),
    ("vmem", ("buffer_", "global_", "flat_", "scratch_")),
]
DESC = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def summarize(path):
    counts, out, sym = collections.defaultdict(collections.Counter), {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"([A-Za-z_][\w$.]*):", s)
        if m and not s.startswith(".L"):
            sym = m.group(1)
        elif s.startswith(".amdhsa_kernel "):
            sym = s.split()[1]
            out[sym] = dict(counts[sym])
        elif s.startswith(".amdhsa_") and sym in out:
            key, _, val = s[len(".amdhsa_"):].partition(" ")
            if key in DESC:
                out[sym][key] = val.strip()
        elif s == ".end_amdhsa_kernel":
            sym = None
        elif sym and s and s[0] not in ".;" and not s.endswith(":"):
            op = s.split()[0]
            counts[sym]["insts"] += 1
            counts[sym][next((c for c, pre in CLASSES if op.startswith(pre)), "other")] += 1
    keys = ["insts"] + [c for c, _ in CLASSES] + ["other"] + list(DESC)
    return {k: " ".join("%s=%s" % (f.replace("_fixed_size", ""), v.get(f, 0)) for f in keys)
            for k, v in out.items()}


def main(argv):
    if len(argv) not in (2, 3, 4):
        sys.exit(__doc__)
    a = summarize(argv[1])
    if len(argv) == 2:
        for k in sorted(a):
            print(k, a[k])
        return 0
    b = summarize(argv[2])
    if len(argv) == 4:
        rename = dict(line.split() for line in open(argv[3]) if line.strip())
        a = {rename.get(k, k): v for k, v in a.items()}
    diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in diff:
        print("%s\n  - %s\n  + %s" % (k, a.get(k, "(absent)"), b.get(k, "(absent)")))
    print("%d / %d kernel symbols, %d differ" % (len(a), len(b), len(diff)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
