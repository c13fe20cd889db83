#!/usr/bin/env python
"""cwbl_analyze_vars (one fused call for a group of variables) against per-variable calls.

Obs set and slabs in device memory, through abi.Core; nvar = 1, 2, 4, 8 distinct variables on
one grid (the workload's var plus device-drawn noise).  One untimed library state first loads
the kernels.  Per nvar and mode, one library state, one untimed repetition (it sizes every
buffer; with record reuse it allocates the cache), then `--reps` timed repetitions.  Each
repetition restores the variables (untimed), starts with a fresh cwbl_set_obs, which clears the
index and record caches, and is timed between two device synchronisations:

  A   nvar cwbl_analyze_var calls, record_reuse at its default: one miss, nvar - 1 hits
  B   the same with record_reuse = 0
  G   one cwbl_analyze_vars(nvar) with record_reuse = 0 (it needs no cache memory)

Printed: median and min-max per mode; reuse_info().bytes_held for A; for B and G the
kernel_times of one further repetition, so the cost of the first and of each further variable
in solve_tq40_multi_kernel can be read off against solve_tq40_kernel; whether the three modes'
analyses are bit-equal; and the condition at the largest nvar: G's median below A's median by
more than A's own min-max range.

  python scripts/analyze_vars_ab.py [--config c2] [--reps 5] [--nvars 1,2,4,8] [--scale S]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402


class Bench:
    def __init__(self, w, nmax):
        import torch
        self.torch, self.w = torch, w
        dev = torch.device("cuda:0")
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.oxyz, self.obs, self.hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
        self.x, self.y, self.alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
        gen = torch.Generator(device=dev).manual_seed(7)
        self.pristine = [to_dev(w.var)]
        for _ in range(1, nmax):
            noise = torch.randn(self.pristine[0].shape, generator=gen, device=dev,
                                dtype=torch.float32)
            self.pristine.append(self.pristine[0] + noise)
        self.vars = [p.clone() for p in self.pristine]
        self.slabs = [abi.make_slab(self.x, self.y, self.alt, v, memory=abi.MEM_DEVICE)
                      for v in self.vars]
        torch.cuda.synchronize()

    def obs_set(self):
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(self.w.radar_type, self.oxyz, self.obs,
                                                           self.hdxb).build()

    def run(self, mode, nvar, reps, keep=None):
        """-> (ms per repetition, bytes_held, kernel_times of one further repetition,
        bit-equal to `keep`'s analyses or None); keep: a list that receives clones of the
        analyses when empty."""
        torch, w = self.torch, self.w
        core = abi.Core(w.k, device=0, options=None if mode == "A" else {"record_reuse": 0})
        vps = [w.vp] * nvar

        def rep():
            for v, p in zip(self.vars[:nvar], self.pristine):
                v.copy_(p)
            core.set_obs(self.obs_set())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "G":
                core.analyze_vars(vps, self.slabs[:nvar])
            else:
                for s in self.slabs[:nvar]:
                    core.analyze_var(w.vp, s)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        rep()  # untimed: buffers sized, the cache allocated
        equal = None
        if keep is not None:
            if not keep:
                keep.extend(v.clone() for v in self.vars[:nvar])
            else:
                equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                            for a, b in zip(self.vars[:nvar], keep))
        ms = [rep() for _ in range(reps)]
        held = core.reuse_info().bytes_held
        core.set_kernel_timing(True)
        rep()
        kt = core.kernel_times()
        core.finalize()
        return ms, held, kt, equal


def stat(ms):
    return f"{np.median(ms):9.3f}  [{min(ms):.3f} .. {max(ms):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nvars", default="1,2,4,8")
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (a quick look)")
    args = ap.parse_args()
    nvars = [int(n) for n in args.nvars.split(",")]
    w = synth.make(args.config, scale=args.scale)
    print(f"== {args.config}: {w.nx}x{w.ny}x{w.nz} grid = {w.points} points, k={w.k}, "
          f"{w.obs.shape[0]} obs{' (scale %g)' % args.scale if args.scale else ''}; "
          f"reps={args.reps}; ms per repetition (all nvar variables), median [min .. max]",
          flush=True)
    b = Bench(w, max(nvars))
    b.run("B", 1, 0)  # untimed: kernels loaded
    b.run("G", 1, 0)
    last = None
    for nvar in nvars:
        keep, res = [], {}
        for mode in ("A", "B", "G"):
            res[mode] = b.run(mode, nvar, args.reps, keep)
        print(f"nvar = {nvar}", flush=True)
        for mode, what in (("A", "analyze_var x nvar, record_reuse default"),
                           ("B", "analyze_var x nvar, record_reuse = 0"),
                           ("G", "analyze_vars(nvar), record_reuse = 0")):
            ms, held, kt, equal = res[mode]
            eq = "" if equal is None else f"   bit-equal to A: {equal}"
            print(f"   {mode}  {stat(ms)}   {what}; bytes_held {held / 2**30:.2f} GiB{eq}")
        for mode in ("B", "G"):
            for name, t in res[mode][2].items():
                if name.startswith(("solve_tq40", "assemble_record")):
                    print(f"      {mode} kernel_times  {name:34s} launches {t['launches']:4d}  "
                          f"points {t['points']:9d}  ms {t['ms']:9.3f}")
        assert res["B"][3] and res["G"][3], "the modes' analyses differ"
        last = (nvar, res)
    nvar, res = last
    a, g = res["A"][0], res["G"][0]
    gap, rng = float(np.median(a) - np.median(g)), max(a) - min(a)
    print(f"condition at nvar = {nvar}: median A - median G = {gap:.3f} ms, A's min-max range "
          f"{rng:.3f} ms: {'met' if gap > rng else 'NOT met'}", flush=True)


if __name__ == "__main__":
    main()
