#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 assembly files of one translation unit (the check of
profiles/twin_merge.txt): python scripts/isa_diff.py PARENT.s NEW.s

Compile both sides with the flags of tests/test_isa_multi.py (hipcc ... --offload-device-only
-S).  Per kernel and side: .vgpr_count, .sgpr_count, .group_segment_fixed_size,
.private_segment_fixed_size and the instruction count; then whether the mnemonic sequences are
equal, and the mnemonics whose counts differ, vector/LDS/memory ones apart from scalar, branch,
nop and waitcnt ones.  A kernel passes where VGPRs, LDS and scratch are equal and no vector, LDS
or memory mnemonic count differs.  Exit status 1 if a kernel does not."""
import collections
import re
import sys

VEC = ("v_", "ds_", "global_", "buffer_", "flat_", "scratch_")
META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def parse(path):
    text = open(path).read()
    kern, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur = m.group(1)
            kern[cur] = {"seq": []}
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur and line.startswith("\t"):
            s = line.strip()
            if s and not s.startswith((".", ";")):
                kern[cur]["seq"].append(s.split()[0])
    for blk in re.split(r"^\s*- \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", blk, re.M).group(1)
        if name in kern:
            for key in META:
                kern[name][key] = int(re.search(r"^\s*\.%s:\s+(\d+)" % key, blk, re.M).group(1))
    return {k: v for k, v in kern.items() if META[0] in v}


def show(side, a):
    print("  %-7s vgpr %3d  sgpr %3d  lds %6d  scratch %3d  instructions %6d" %
          ((side,) + tuple(a[k] for k in META) + (len(a["seq"]),)))


def main():
    A, B = parse(sys.argv[1]), parse(sys.argv[2])
    ok = set(A) == set(B)
    for k in sorted(set(A) ^ set(B)):
        print("%s: on one side only" % k)
    for k in sorted(set(A) & set(B)):
        a, b = A[k], B[k]
        print(k)
        show("parent", a)
        show("new", b)
        ha, hb = collections.Counter(a["seq"]), collections.Counter(b["seq"])
        d = {m: hb[m] - ha[m] for m in set(ha) | set(hb) if ha[m] != hb[m]}
        vec = sorted((m, v) for m, v in d.items() if m.startswith(VEC))
        oth = sorted((m, v) for m, v in d.items() if not m.startswith(VEC))
        same = a["seq"] == b["seq"]
        res = all(a[x] == b[x] for x in META if x != "sgpr_count")
        fmt = lambda l: ", ".join("%s %+d" % e for e in l) or "none"  # noqa: E731
        print("  mnemonic sequence identical: %s" % ("yes" if same else "no"))
        print("  vector/LDS/memory mnemonic differences: %s" % fmt(vec))
        print("  scalar/branch/nop/waitcnt differences: %s" % fmt(oth))
        good = res and not vec
        print("  gate 1: %s%s" % ("pass" if good else "FAIL",
                                  " (identical stream: no timing needed)" if good and same else ""))
        ok &= good
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
