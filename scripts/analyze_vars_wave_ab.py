#!/usr/bin/env python
"""cwbl_analyze_vars at an ensemble size of the one-wavefront path (k <= 16, 41..64), for an
A/B of two builds of the library.

One run measures one library (CWBL_LIBRARY, or the tree's own): per nvar one library state, one
untimed repetition, then `--reps` timed ones of one cwbl_analyze_vars(nvar) call; each
repetition restores the variables (untimed), starts with a fresh cwbl_set_obs (index cache
cleared) and is timed between two device synchronisations.  Printed per nvar: median and
min-max, the kernel_times of one further repetition, and a SHA-256 of every variable's
analysis.  `--digests FILE` writes the digests when FILE does not exist and compares with it
otherwise, so that a second run (another build, the same inputs) reports bit-equality at full
size.  Run the two builds alternately in one session (profiles/analyze_vars_wave.txt):

  CWBL_LIBRARY=<parent>/libcwbl.so python scripts/analyze_vars_wave_ab.py --k 64 --label B \\
      --digests d64.json
  python scripts/analyze_vars_wave_ab.py --k 64 --label G --digests d64.json
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from analyze_vars_ab import Bench, stat  # noqa: E402
from cwbl import abi, synth  # noqa: E402


def run(b, nvar, reps):
    torch, w = b.torch, b.w
    core = abi.Core(w.k, device=0)
    vps = [w.vp] * nvar

    def rep():
        for v, p in zip(b.vars[:nvar], b.pristine):
            v.copy_(p)
        core.set_obs(b.obs_set())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        core.analyze_vars(vps, b.slabs[:nvar])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rep()  # untimed: buffers sized
    digests = [hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for v in b.vars[:nvar]]
    ms = [rep() for _ in range(reps)]
    core.set_kernel_timing(True)
    rep()
    kt = core.kernel_times()
    core.finalize()
    return ms, kt, digests


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nvars", default="1,2,4,8")
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (a quick look)")
    ap.add_argument("--label", default="G")
    ap.add_argument("--digests", default=None)
    args = ap.parse_args()
    nvars = [int(n) for n in args.nvars.split(",")]
    w = synth.make(args.config, scale=args.scale, k=args.k)
    print(f"== {args.label}: {args.config} {w.nx}x{w.ny}x{w.nz} = {w.points} points, k={w.k}, "
          f"{w.obs.shape[0]} obs; reps={args.reps}; library "
          f"{os.environ.get('CWBL_LIBRARY', '(this tree)')}; ms per call (all nvar variables), "
          f"median [min .. max]", flush=True)
    b = Bench(w, max(nvars))
    run(b, 1, 0)  # untimed: kernels loaded
    if max(nvars) > 1:
        run(b, 2, 0)
    found = {}
    for nvar in nvars:
        ms, kt, found[str(nvar)] = run(b, nvar, args.reps)
        print(f"   {args.label} nvar = {nvar}  {stat(ms)}", flush=True)
        for name, t in kt.items():
            if name.startswith(("solve_", "search_", "tune_q")):
                print(f"      {args.label} kernel_times  {name:34s} launches {t['launches']:4d}  "
                      f"points {t['points']:9d}  ms {t['ms']:9.3f}")
    if args.digests:
        if os.path.exists(args.digests):
            want = json.load(open(args.digests))
            for n in found:
                print(f"   {args.label} nvar = {n}  bit-equal to {args.digests}: "
                      f"{found[n] == want.get(n)}", flush=True)
            assert all(found[n] == want.get(n) for n in found), "the analyses differ"
        else:
            json.dump(found, open(args.digests, "w"))
            print(f"   {args.label} digests written to {args.digests}")


if __name__ == "__main__":
    main()
