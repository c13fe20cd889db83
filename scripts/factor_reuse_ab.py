#!/usr/bin/env python
"""What the record cache keeps (CWBL_OPT_FACTOR_REUSE), by the bench headline's procedure.

One run measures one library (CWBL_LIBRARY, or the tree's own).  Obs set and slab in device
memory, `--warmup` untimed calls, then `--steps` calls timed as one block between two device
synchronisations (bench.py's timed region), through abi.Core.  Per mode

  off       record_reuse = 0: every call runs the QC columns, the search and the assembly
  records   factor_reuse = 0: the cache keeps records, a hit runs solve_tq40_kernel
  factors   the default: the cache keeps factors, a hit runs solve_tq40_factor_kernel

it prints the warm ms per step (median [min .. max] over `--reps` timed blocks), and over
`--reps` further cwbl_set_obs calls the fill call (the first call after cwbl_set_obs: a miss
that refills the cache), the hit after it and their sum.  A library without the option (an
older build) is measured in the modes `off` and `as built`.

  python scripts/factor_reuse_ab.py [--config c2] [--steps 20] [--warmup 5] [--reps 3] [--scale S]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402

OPTIONS = {"off": {"record_reuse": 0}, "records": {"factor_reuse": 0}, "factors": None,
           "as built": None}


def has_option():
    c = abi.Core(40, device=0)
    try:
        c.set_option("factor_reuse", 1)
        return True
    except abi.CwblError:
        return False
    finally:
        c.finalize()


def measure(w, mode, steps, warmup, reps):
    import torch
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
    var = to_dev(w.var)
    torch.cuda.synchronize()
    core = abi.Core(w.k, device=0, options=OPTIONS[mode])
    slab = abi.make_slab(x, y, alt, var, memory=abi.MEM_DEVICE)

    def obs_set():
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(w.radar_type, oxyz, obs, hdxb).build()

    def timed(n=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            core.analyze_var(w.vp, slab)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    core.set_obs(obs_set())
    for _ in range(warmup):
        core.analyze_var(w.vp, slab)
    r = {"warm": [timed(steps) for _ in range(reps)], "fill": [], "hit": []}
    r["warm_info"] = core.reuse_info().as_dict()
    for _ in range(reps):
        core.set_obs(obs_set())
        r["fill"].append(timed())
        r["fill_info"] = core.reuse_info().as_dict()
        r["hit"].append(timed())
    core.finalize()
    return r


def spread(v):
    return f"{np.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (trial runs)")
    args = ap.parse_args()
    w = synth.make(args.config, scale=args.scale)
    print(f"== {args.config}: {w.nx}x{w.ny}x{w.nz} grid, k={w.k}, {w.obs.shape[0]} obs"
          f"{' (scale %g)' % args.scale if args.scale else ''}; steps={args.steps} "
          f"warmup={args.warmup} reps={args.reps}; library "
          f"{os.environ.get('CWBL_LIBRARY', '(this tree)')}", flush=True)
    modes = ("off", "records", "factors") if has_option() else ("off", "as built")
    measure(w, "off", 1, 1, 0)  # untimed: kernels loaded
    for mode in modes:
        r = measure(w, mode, args.steps, args.warmup, args.reps)
        both = [f + h for f, h in zip(r["fill"], r["hit"])]
        wi, fi = r["warm_info"], r["fill_info"]
        print(f"{mode}:")
        print(f"   warm ms per step {spread(r['warm'])}   reused={wi['batches_reused']} "
              f"assembled={wi['batches_assembled']} held={wi['bytes_held'] / 2**30:.2f} GiB")
        print(f"   fill call        {spread(r['fill'])}   reused={fi['batches_reused']} "
              f"assembled={fi['batches_assembled']}")
        print(f"   hit after it     {spread(r['hit'])}")
        print(f"   fill + hit       {spread(both)}", flush=True)


if __name__ == "__main__":
    main()
