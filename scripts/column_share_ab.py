#!/usr/bin/env python
"""CWBL_OPT_COLUMN_SHARE against the per-point call, on a variable with 2-D localisation.

The C2 grid with vclr = -1 (no obs type localises vertically) and --nz levels, at each --ks
ensemble size; obs set and slab in device memory, through abi.Core.  Per k, one process, the
modes alternated --rounds times:

  P   the library --parent names (the parent commit's build), column_share not set
  0   this tree's library, column_share = 0: the per-point call
  1   column_share = 1: the column kernel (k = 17..40) or the level-chunked group kernels
  2   column_share = 2: the level-chunked group kernels on the record path too
  F   (--factor, in mode 2's place) column_share = 1 with column_factor = 1: every level from
      one kept factor per column (k = 41..96); the output goes to profiles/column_factor.txt.
      At k = 97, 112, 128 (any k > 96) mode F sets column_rows = 1 as well, which makes that
      class eligible; mode 1 is then the same call without column_rows (the level chunks), mode
      P1 the parent's library with column_share = 1 (column_rows = 0 costs nothing), and the
      output goes to profiles/column_rows.txt

Every mode runs with record_reuse = 0 (a shared call runs without the cache; the per-point
call then pays no cache fill either).  Per mode and round: one library state, one untimed
repetition (it sizes every buffer), then --reps timed ones; each restores the variable
(untimed), starts with a fresh cwbl_set_obs, which clears the index cache, and is timed between
two device synchronisations.  Printed per k: median and min-max per mode over both rounds, the
SHA-256 of the analysed slab (it must agree across all modes), column_info, the kernel_times
of one further repetition per mode, the ratios of modes 1 and 2 to mode 0 of the same session,
and whether P and 0 agree within their run-to-run ranges (option 0 costs nothing).  With
--factor also mode F / mode 1 and whether F is faster than 1 by more than either mode's
run-to-run range (the bar of the option's eligibility at that k).

  python scripts/column_share_ab.py [--ks 40,64,96] [--nz 50] [--reps 3] [--rounds 2]
                                    [--parent DIR/libcwbl.so] [--scale S] [--out FILE]
                                    [--factor]
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402

OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


class Bench:
    def __init__(self, w):
        import torch
        self.torch, self.w = torch, w
        dev = torch.device("cuda:0")
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.oxyz, self.obs, self.hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
        self.x, self.y, self.alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
        self.pristine = to_dev(w.var)
        self.var = self.pristine.clone()
        self.slab = abi.make_slab(self.x, self.y, self.alt, self.var, memory=abi.MEM_DEVICE)
        torch.cuda.synchronize()

    def obs_set(self):
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(self.w.radar_type, self.oxyz, self.obs,
                                                           self.hdxb).build()

    def run(self, lib, share, reps, digest, kernels):
        """-> (ms per repetition, SHA-256 of the analysis or None, column_info or None,
        kernel_times of one further repetition or None).  share "F": 1 with column_factor."""
        torch, w = self.torch, self.w
        opts = {"record_reuse": 0}
        if share == "F":
            opts.update(column_share=1, column_factor=1)
            if w.k > 96:
                opts["column_rows"] = 1
        elif share == "P1":
            opts["column_share"] = 1
        elif share is not None:
            opts["column_share"] = share
        core = abi.Core(w.k, device=0, lib=lib, options=opts)

        def rep():
            self.var.copy_(self.pristine)
            core.set_obs(self.obs_set())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            core.analyze_var(w.vp, self.slab)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        rep()  # untimed: buffers sized
        sha = hashlib.sha256(self.var.cpu().numpy().tobytes()).hexdigest() if digest else None
        info = core.column_info().as_dict() if share is not None else None
        ms = [rep() for _ in range(reps)]
        kt = None
        if kernels:
            core.set_kernel_timing(True)
            rep()
            kt = core.kernel_times()
        core.finalize()
        return ms, sha, info, kt


def stat(ms):
    return f"{np.median(ms):10.3f}  [{min(ms):.3f} .. {max(ms):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="40,64,96")
    ap.add_argument("--nz", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="the parent commit's libcwbl.so (mode P)")
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (a quick look)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--factor", action="store_true", help="mode F in mode 2's place")
    args = ap.parse_args()
    ks = [int(s) for s in args.ks.split(",")]
    rows = args.factor and max(ks) > 96
    if args.out is None:
        args.out = os.path.join(REPO, "profiles",
                                "column_rows.txt" if rows else
                                "column_factor.txt" if args.factor else "column_share.txt")
    here = abi.load_library()
    modes = [("0", here, 0), ("1", here, 1),
             ("F", here, "F") if args.factor else ("2", here, 2)]
    if args.parent:
        # (the parent lacks this change's entry points: the prototypes of those it has)
        import ctypes
        parent = ctypes.CDLL(os.path.abspath(args.parent))
        for name in abi.EXPORTS:
            if hasattr(parent, name):
                fn, ours = getattr(parent, name), getattr(here, name)
                fn.argtypes, fn.restype = ours.argtypes, ours.restype
        modes.insert(0, ("P", parent, None))
        if rows:
            modes.insert(1, ("P1", parent, "P1"))
    what = {"P": "parent commit's library", "0": "column_share = 0 (per point)",
            "1": "column_share = 1", "2": "column_share = 2 (level chunks)",
            "F": "column_share = 1, column_factor = 1",
            "P1": "parent commit's library, column_share = 1"}
    if rows:
        what["F"] += ", column_rows = 1 above k = 96"
    for k in ks:
        w = synth.make("c2", k=k, nz=args.nz, vclr=-1.0, scale=args.scale)
        say(f"== c2, vclr = -1: {w.nx}x{w.ny}x{w.nz} grid = {w.points} points, k={k}, "
            f"{w.obs.shape[0]} obs{' (scale %g)' % args.scale if args.scale else ''}; "
            f"record_reuse = 0; reps={args.reps} x rounds={args.rounds}; ms per call, "
            f"median [min .. max]")
        b = Bench(w)
        b.run(here, 0, 0, False, False)  # untimed: kernels loaded
        res = {m: dict(ms=[], sha=None, info=None, kt=None) for m, _, _ in modes}
        for rnd in range(args.rounds):
            for m, lib, share in modes:
                last = rnd == args.rounds - 1
                ms, sha, info, kt = b.run(lib, share, args.reps, rnd == 0, last)
                r = res[m]
                r["ms"] += ms
                r["sha"], r["info"], r["kt"] = sha or r["sha"], info or r["info"], kt or r["kt"]
        for m, _, _ in modes:
            r = res[m]
            say(f"   {m}  {stat(r['ms'])}   {what[m]}")
            say(f"      sha256 {r['sha']}")
            if r["info"]:
                say(f"      column_info {r['info']}")
            for name, t in r["kt"].items():
                say(f"      kernel_times  {name:40s} launches {t['launches']:4d}  "
                    f"points {t['points']:10d}  ms {t['ms']:10.3f}")
        shas = {r["sha"] for r in res.values()}
        say(f"   analyses bit-equal across the modes: {len(shas) == 1}")
        m0 = float(np.median(res["0"]["ms"]))
        last = modes[-1][0]  # "2" or "F"
        for m in ("1", last):
            mm = float(np.median(res[m]["ms"]))
            say(f"   mode {m} / mode 0 = {mm / m0:.3f}  ({'below' if mm < 0.5 * m0 else 'NOT below'} "
                f"half of mode 0)")
        m1, m2 = (float(np.median(res[m]["ms"])) for m in ("1", last))
        if args.factor:
            one, fac = res["1"]["ms"], res["F"]["ms"]
            rng = max(max(one) - min(one), max(fac) - min(fac))
            say(f"   mode F / mode 1 = {m2 / m1:.3f}; median 1 - median F = {m1 - m2:.3f} ms, "
                f"run-to-run range {rng:.3f} ms: F is "
                f"{'faster' if m1 - m2 > rng else 'NOT faster'} by more than the range")
        else:
            say(f"   mode 1 / mode 2 = {m1 / m2:.3f}")
        if "P" in res:
            p, z = res["P"]["ms"], res["0"]["ms"]
            gap = abs(float(np.median(p) - np.median(z)))
            rng = max(max(p) - min(p), max(z) - min(z))
            say(f"   |median P - median 0| = {gap:.3f} ms, run-to-run range {rng:.3f} ms: "
                f"{'within' if gap <= rng else 'NOT within'}")
        if "P1" in res:
            p, z = res["P1"]["ms"], res["1"]["ms"]
            gap = abs(float(np.median(p) - np.median(z)))
            say(f"   |median P1 - median 1| = {gap:.3f} ms, the parent's own range "
                f"{max(p) - min(p):.3f} ms: {'within' if gap <= max(p) - min(p) else 'NOT within'}")
        say()
        del b
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every k: a later failure keeps what ran)
            f.write("\n".join(OUT) + "\n")
        assert len(shas) == 1, "the modes' analyses differ"


if __name__ == "__main__":
    main()
