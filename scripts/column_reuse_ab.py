#!/usr/bin/env python
"""CWBL_OPT_COLUMN_REUSE on the MU -> P -> PH sequence: three variables of one 2-D localisation
whose slabs share x and y and differ in nz (1, nz, nz + 1) and alt.

The C2 grid with vclr = -1 and --nz levels (the three calls analyse the levels [0, 1), [0, nz)
and [0, nz + 1) of one var array, each with an alt array of its own), at each --ks ensemble size;
obs set and slabs in device memory, through abi.Core.  column_share = 1, with column_factor = 1
above k = 40, and record_reuse = 0 in every mode.  Per k, one process, the modes alternated
--rounds times:

  P   the library --parent names (the parent commit's build), column_reuse not set
  0   this tree's library, column_reuse = 0
  R   column_reuse = --budget MiB: MU fills the column cache, P and PH hit it

At k = 97, 112, 128 (any k > 96) modes 0 and R set column_rows = 1 as well, which makes that
class eligible for both options: mode 0 is then the shared call from the workspace of
column_factor, mode P (the parent's library, which has no such option) the level chunks, and the
output is appended to profiles/column_rows.txt behind scripts/column_share_ab.py --factor's.

Per mode and round: one Core for the whole sequence, one untimed repetition (it sizes every
buffer), then --reps timed ones.  A repetition restores the three variables (untimed) and starts
with a fresh cwbl_set_obs, which clears the index cache and voids the column cache, so that the
MU call of every repetition is a fill; each call is timed between two device synchronisations.
Printed per k and call: median and min-max per mode over all rounds, the SHA-256 of the analysed
slab (it must agree across the modes), column_info, column_reuse_info with the bytes held, and
the kernel_times of one further repetition.  Then the bars: a hit (P and PH under R) is faster
than the same call under 0 by more than either mode's run-to-run range, and 0 agrees with the
parent within the parent's run-to-run range.

  python scripts/column_reuse_ab.py [--ks 40,64,96] [--nz 50] [--reps 3] [--rounds 2]
                                    [--budget 16384] [--parent DIR/libcwbl.so] [--scale S]
                                    [--out FILE]
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
NAMES = ("MU", "P", "PH")


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


class Bench:
    def __init__(self, w, nz):
        import torch
        self.torch, self.w = torch, w
        dev = torch.device("cuda:0")
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.oxyz, self.obs, self.hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
        self.x, self.y = to_dev(w.x), to_dev(w.y)
        self.levels = (1, nz, nz + 1)
        self.pristine = to_dev(w.var)  # (k, nz + 1, ny, nx)
        self.vars, self.slabs = [], []
        for n in self.levels:
            # (a copy of its own: the deepest slab would otherwise be pristine itself)
            var = self.pristine[:, :n].clone(memory_format=torch.contiguous_format)
            alt = to_dev(w.alt[:n] + np.float32(n))
            self.vars.append(var)
            self.slabs.append(abi.make_slab(self.x, self.y, alt, var, memory=abi.MEM_DEVICE))
        torch.cuda.synchronize()

    def obs_set(self):
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(self.w.radar_type, self.oxyz, self.obs,
                                                           self.hdxb).build()

    def run(self, lib, budget, reps, digest, kernels):
        """One Core, the sequence reps times -> per call: ms list, SHA-256, column_info,
        column_reuse_info, kernel_times of one further repetition (None where not asked)."""
        torch, w = self.torch, self.w
        opts = {"record_reuse": 0, "column_share": 1}
        if w.k > 40:
            opts["column_factor"] = 1
        if budget is not None:
            opts["column_reuse"] = budget
            if w.k > 96:  # (this tree's library only: the parent has no such option)
                opts["column_rows"] = 1
        core = abi.Core(w.k, device=0, lib=lib, options=opts)
        has_info = hasattr(lib, "cwbl_column_reuse_info")

        def rep(kt=None, infos=None):
            for var, n in zip(self.vars, self.levels):
                var.copy_(self.pristine[:, :n])
            core.set_obs(self.obs_set())
            ms = []
            for i, slab in enumerate(self.slabs):
                if kt is not None:
                    core.set_kernel_timing(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                core.analyze_var(w.vp, slab)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                if kt is not None:
                    kt.append(core.kernel_times())
                if infos is not None:
                    infos.append((core.column_info().as_dict(),
                                  core.column_reuse_info().as_dict() if has_info else None))
            return ms

        infos = []
        rep(infos=infos)  # untimed: buffers sized
        sha = [hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for v in self.vars] \
            if digest else None
        ms = [rep() for _ in range(reps)]
        kt = None
        if kernels:
            kt = []
            rep(kt=kt)
            core.set_kernel_timing(False)
        core.finalize()
        return [[m[i] for m in ms] for i in range(3)], sha, infos, kt


def stat(ms):
    return f"{np.median(ms):10.3f}  [{min(ms):.3f} .. {max(ms):.3f}]"


def spread(ms):
    return max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="40,64,96")
    ap.add_argument("--nz", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--budget", type=int, default=16384, help="column_reuse of mode R, MiB")
    ap.add_argument("--parent", default=None, help="the parent commit's libcwbl.so (mode P)")
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (a quick look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = [int(s) for s in args.ks.split(",")]
    rows = max(ks) > 96
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "column_rows.txt" if rows else "column_reuse.txt")
    before = ""
    if rows and os.path.exists(args.out):
        with open(args.out) as f:
            before = f.read()
    here = abi.load_library()
    modes = [("0", here, 0), ("R", here, args.budget)]
    if args.parent:
        # (the parent lacks this change's entry point: the prototypes of those it has)
        import ctypes
        parent = ctypes.CDLL(os.path.abspath(args.parent))
        for name in abi.EXPORTS:
            if hasattr(parent, name):
                fn, ours = getattr(parent, name), getattr(here, name)
                fn.argtypes, fn.restype = ours.argtypes, ours.restype
        modes.insert(0, ("P", parent, None))
    what = {"P": "parent commit's library", "0": "column_reuse = 0",
            "R": f"column_reuse = {args.budget} MiB"}
    failed = []
    for k in ks:
        w = synth.make("c2", k=k, nz=args.nz + 1, vclr=-1.0, scale=args.scale)
        say(f"== c2, vclr = -1: {w.nx}x{w.ny} columns = {w.nx * w.ny}, nz = 1, {args.nz}, "
            f"{args.nz + 1}, k={k}, {w.obs.shape[0]} obs"
            f"{' (scale %g)' % args.scale if args.scale else ''}; column_share = 1"
            f"{', column_factor = 1' if k > 40 else ''}"
            f"{', column_rows = 1 (modes 0 and R)' if k > 96 else ''}, record_reuse = 0; "
            f"reps={args.reps} x "
            f"rounds={args.rounds}; ms per call, median [min .. max]")
        b = Bench(w, args.nz)
        b.run(here, 0, 0, False, False)  # untimed: kernels loaded
        res = {m: dict(ms=[[], [], []], sha=None, infos=None, kt=None) for m, _, _ in modes}
        for rnd in range(args.rounds):
            for m, lib, budget in modes:
                ms, sha, infos, kt = b.run(lib, budget, args.reps, rnd == 0,
                                           rnd == args.rounds - 1)
                r = res[m]
                for i in range(3):
                    r["ms"][i] += ms[i]
                r["sha"], r["infos"], r["kt"] = sha or r["sha"], infos, kt or r["kt"]
        for i, name in enumerate(NAMES):
            say(f" {name} (nz = {b.levels[i]})")
            for m, _, _ in modes:
                r = res[m]
                say(f"   {m}  {stat(r['ms'][i])}   {what[m]}")
                say(f"      sha256 {r['sha'][i]}")
                info, reuse = r["infos"][i]
                say(f"      column_info {info}")
                if reuse is not None:
                    say(f"      column_reuse_info {reuse}")
                for kn, t in r["kt"][i].items():
                    say(f"      kernel_times  {kn:48s} launches {t['launches']:4d}  "
                        f"points {t['points']:10d}  ms {t['ms']:10.3f}")
            equal = len({res[m]["sha"][i] for m, _, _ in modes}) == 1
            say(f"   analyses bit-equal across the modes: {equal}")
            if not equal:
                failed.append(f"k={k} {name}: the modes' analyses differ")
            zero, hit = res["0"]["ms"][i], res["R"]["ms"][i]
            gain = float(np.median(zero) - np.median(hit))
            rng = max(spread(zero), spread(hit))
            if i > 0:
                ok = gain > rng
                say(f"   hit / miss = {np.median(hit) / np.median(zero):.3f}; median 0 - median R"
                    f" = {gain:.3f} ms, run-to-run range {rng:.3f} ms: a hit is "
                    f"{'faster' if ok else 'NOT faster'} by more than the range")
            else:
                say(f"   fill / miss = {np.median(hit) / np.median(zero):.3f} (the fill is a "
                    f"shared call of one level; the miss is the per-point call)")
            if "P" in res and k > 96:
                p = res["P"]["ms"][i]
                say(f"   mode 0 / mode P = {np.median(zero) / np.median(p):.3f} (P: the level "
                    f"chunks, or for MU the per-point call)")
            elif "P" in res:
                p = res["P"]["ms"][i]
                gap = abs(float(np.median(p) - np.median(zero)))
                say(f"   |median P - median 0| = {gap:.3f} ms, the parent's run-to-run range "
                    f"{spread(p):.3f} ms: {'within' if gap <= spread(p) else 'NOT within'}")
        say()
        del b
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every k: a later failure keeps what ran)
            f.write(before + "\n".join(OUT) + "\n")
    assert not failed, failed


if __name__ == "__main__":
    main()
