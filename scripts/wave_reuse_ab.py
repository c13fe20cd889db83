#!/usr/bin/env python
"""The factor cache of the one-wavefront path (CWBL_OPT_WAVE_REUSE, k = 41..64), by the bench
headline's procedure.

One run measures one library (CWBL_LIBRARY, or the tree's own).  Obs set and slab in device
memory, `--warmup` untimed calls, then `--steps` calls timed as one block between two device
synchronisations (bench.py's timed region), through abi.Core.  Per mode

  off   the option absent: every call runs the QC columns, the search and solve_tq_kernel
  on    wave_reuse = 1 (and record_reuse = --budget MiB when given): a miss runs
        fill_tq_wave_kernel, a hit solve_tq_wave_factor_kernel alone

it prints the warm ms per call (median [min .. max] over `--reps` timed blocks; under `on` these
calls are hits), and over `--reps` further cwbl_set_obs calls the first call after cwbl_set_obs
(under `on` a miss that refills the cache), the call after it and their sum; then the kernel
times of one more warm call and, for a hit, the rate at which its kernel streams the factors.
A library without the option (an older build) is measured in the mode `off` alone.

  python scripts/wave_reuse_ab.py [--config c2] [--k 64] [--budget MiB] [--steps 5]
                                  [--warmup 2] [--reps 3] [--scale S]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402

WAVE_REUSE = 19  # by number: an older abi.py has no name for it


def has_option():
    c = abi.Core(64, device=0)
    try:
        c.set_option(WAVE_REUSE, 1)
        return True
    except abi.CwblError:
        return False
    finally:
        c.finalize()


def factor_bytes(k):
    kp = (k + 7) // 8 * 8
    return 8 * (kp * (kp - 1) // 2 + 5 * kp)


def measure(w, mode, budget, steps, warmup, reps):
    import torch
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
    var = to_dev(w.var)
    torch.cuda.synchronize()
    core = abi.Core(w.k, device=0)
    if mode == "on":
        if budget:
            core.set_option("record_reuse", budget)
        core.set_option(WAVE_REUSE, 1)
    slab = abi.make_slab(x, y, alt, var, memory=abi.MEM_DEVICE)

    def obs_set():
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(w.radar_type, oxyz, obs, hdxb).build()

    def timed(n=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            st = core.analyze_var(w.vp, slab)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, st

    core.set_obs(obs_set())
    for _ in range(warmup):
        core.analyze_var(w.vp, slab)
    r = {"warm": [timed(steps)[0] for _ in range(reps)], "first": [], "second": []}
    r["warm_info"] = core.reuse_info().as_dict()
    for _ in range(reps):
        core.set_obs(obs_set())
        r["first"].append(timed()[0])
        r["first_info"] = core.reuse_info().as_dict()
        r["second"].append(timed()[0])
    core.set_kernel_timing(True)
    _, st = timed()
    r["kernels"] = core.kernel_times()
    r["solved"] = st.solved
    core.finalize()
    return r


def spread(v):
    return f"{np.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--budget", type=int, default=0, help="record_reuse in MiB (0: the default)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (trial runs)")
    args = ap.parse_args()
    w = synth.make(args.config, scale=args.scale, k=args.k)
    print(f"== {args.config}: {w.nx}x{w.ny}x{w.nz} grid, k={w.k}, {w.obs.shape[0]} obs"
          f"{' (scale %g)' % args.scale if args.scale else ''}; budget "
          f"{args.budget or 'default'} MiB; steps={args.steps} warmup={args.warmup} "
          f"reps={args.reps}; library {os.environ.get('CWBL_LIBRARY', '(this tree)')}", flush=True)
    modes = ("off", "on") if has_option() else ("off",)
    measure(w, "off", 0, 1, 1, 0)  # untimed: kernels loaded
    for mode in modes:
        r = measure(w, mode, args.budget, args.steps, args.warmup, args.reps)
        both = [f + h for f, h in zip(r["first"], r["second"])]
        wi, fi = r["warm_info"], r["first_info"]
        print(f"{mode}:")
        print(f"   warm ms per call    {spread(r['warm'])}   reused={wi['batches_reused']} "
              f"assembled={wi['batches_assembled']} held={wi['bytes_held'] / 2**30:.2f} GiB")
        print(f"   call after set_obs  {spread(r['first'])}   reused={fi['batches_reused']} "
              f"assembled={fi['batches_assembled']}")
        print(f"   call after it       {spread(r['second'])}")
        print(f"   sum of the two      {spread(both)}")
        for name, t in sorted(r["kernels"].items()):
            line = f"   {name:42s} {t['launches']:4d} launches {t['points']:9d} points {t['ms']:9.3f} ms"
            if name.startswith("solve_tq_wave_factor_kernel") and t["ms"] > 0:
                # points with p = 0 read their info alone
                share = t["points"] / max(1, w.points)
                gb = r["solved"] * share * factor_bytes(w.k) / 1e9
                line += f"   {gb:.1f} GB of factors at {gb / t['ms']:.2f} TB/s"
            print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
