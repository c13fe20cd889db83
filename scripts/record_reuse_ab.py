#!/usr/bin/env python
"""Record reuse (CWBL_OPT_RECORD_REUSE) off against on, by the bench headline's procedure.

Obs set and slab in device memory, `--warmup` untimed calls, then `--steps` calls timed as one
block between two device synchronisations (bench.py's timed region), through abi.Core.  Per
mode ("off": record_reuse = 0; "on": the default budget) it prints

  warm ms per step   with reuse on every timed call is a hit, as in the bench; with it off
                     every call runs the QC columns, the search and the assembly
  first call         the library state's first cwbl_analyze_var: sizes every buffer and, with
                     reuse on, allocates the record cache
  fill call          the first call after a further cwbl_set_obs (`--reps` of them): a miss
                     that refills the cache, the allocation already held
  allocation         first call - fill call; "off" gives the share of the ordinary buffers,
                     the rest of "on" is the cache's one-off allocation
  reuse_info         of the last warm call and of the last fill call

One untimed library state first loads the kernels.  A library without the option (an older
build) is measured once, as it is.

  python scripts/record_reuse_ab.py [--config c2] [--steps 10] [--warmup 3] [--reps 3] [--scale S]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402

HAS_REUSE = "record_reuse" in abi.OPTIONS


def measure(w, mode, steps, warmup, reps):
    import torch
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
    var = to_dev(w.var)
    torch.cuda.synchronize()
    core = abi.Core(w.k, device=0, options={"record_reuse": 0} if mode == "off" else None)
    slab = abi.make_slab(x, y, alt, var, memory=abi.MEM_DEVICE)

    def obs_set():
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(w.radar_type, oxyz, obs, hdxb).build()

    def timed(fn, n=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    def info():
        return core.reuse_info().as_dict() if HAS_REUSE else None

    call = lambda: core.analyze_var(w.vp, slab)  # noqa: E731
    core.set_obs(obs_set())
    r = {}
    r["first"], _ = timed(call)
    for _ in range(warmup - 1):
        call()
    r["warm"], st = timed(call, steps)
    r["warm_info"], r["warm_stats"] = info(), st
    r["fill"] = []
    for _ in range(reps):
        core.set_obs(obs_set())
        ms, st = timed(call)
        r["fill"].append(ms)
        r["fill_info"], r["fill_stats"] = info(), st
        call()
    core.finalize()
    return r


def fmt_info(i):
    if i is None:
        return "n/a"
    return (f"reused={i['batches_reused']} assembled={i['batches_assembled']} "
            f"held={i['bytes_held'] / 2**30:.2f} GiB ms_compare={i['ms_compare']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (trial runs)")
    args = ap.parse_args()
    w = synth.make(args.config, scale=args.scale)
    print(f"== {args.config}: {w.nx}x{w.ny}x{w.nz} grid, k={w.k}, {w.obs.shape[0]} obs"
          f"{' (scale %g)' % args.scale if args.scale else ''}; steps={args.steps} "
          f"warmup={args.warmup} reps={args.reps}", flush=True)
    measure(w, "off" if HAS_REUSE else "as built", 1, 1, 0)  # untimed: kernels loaded
    res = {}
    for mode in (("off", "on") if HAS_REUSE else ("as built",)):
        r = res[mode] = measure(w, mode, args.steps, args.warmup, args.reps)
        fill = float(np.median(r["fill"])) if r["fill"] else float("nan")
        s = r["warm_stats"]
        print(f"record_reuse {mode}:", flush=True)
        print(f"   warm ms per step   {r['warm']:9.3f}   (ms_prep {s.ms_prep:.3f}, ms_search "
              f"{s.ms_search:.3f}, ms_solve {s.ms_solve:.3f} of the last)")
        print(f"   first call         {r['first']:9.3f}")
        print(f"   fill call          {fill:9.3f}   after cwbl_set_obs, median of "
              + " ".join(f"{v:.3f}" for v in r["fill"]))
        print(f"   allocation         {r['first'] - fill:9.3f}   first call - fill call")
        print(f"   reuse_info, warm   {fmt_info(r['warm_info'])}")
        print(f"   reuse_info, fill   {fmt_info(r['fill_info'])}")
        print(f"   solved={s.solved} nobs_sum={s.nobs_sum} lz_truncated={s.lz_truncated}", flush=True)
    if HAS_REUSE:
        for key in ("solved", "nobs_sum", "lz_truncated", "sweeps_sum", "max_p"):
            a, b = (getattr(res[m]["warm_stats"], key) for m in ("off", "on"))
            assert a == b, (key, a, b)
        off, on = res["off"], res["on"]
        print(f"warm step, on / off: {on['warm']:.3f} / {off['warm']:.3f} ms = "
              f"{on['warm'] / off['warm']:.3f}; fill call, on / off: "
              f"{np.median(on['fill']):.3f} / {np.median(off['fill']):.3f} ms; cache allocation: "
              f"{(on['first'] - np.median(on['fill'])) - (off['first'] - np.median(off['fill'])):.1f} ms",
              flush=True)


if __name__ == "__main__":
    main()
