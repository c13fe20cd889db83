#!/usr/bin/env python
"""The factor cache of the hand-off path (CWBL_OPT_BIG_REUSE at k = 65..96, CWBL_OPT_ROWS_REUSE
at k = 97..128: the option is picked by the ensemble size's KP), by the bench headline's
procedure.

One run measures one library (CWBL_LIBRARY, or the tree's own).  Obs set and slab in device
memory, `--warmup` untimed calls, then `--steps` calls timed as one block between two device
synchronisations (bench.py's timed region), through abi.Core.  Per mode

  off   the option absent: every call runs the QC columns, the search, the hand-off kernel and
        solve_tqb_tail_kernel
  on    the option = 1 and record_reuse = --budget MiB (the largest of --budget's values whose
        allocation succeeds): a miss runs the hand-off kernel and fill_tqb_tail_kernel, a hit
        solve_tqb_factor_kernel alone over the cached batches

it prints the warm ms per call (median [min .. max] over `--reps` timed blocks; under `on` these
calls are hits), and over `--reps` further cwbl_set_obs calls the first call after cwbl_set_obs
(under `on` a miss that refills the cache), the call after it and their sum; then the kernel
times of one more warm call, for a hit the rate at which its kernel streams the factors and the
hit kernel's time per cached batch, and the SHA-256 of the analysis of the workload's variable
by a warm call and (on) by the fill and the hit after it.  A library without the option (an
older build) is measured in the mode `off` alone.

  python scripts/big_reuse_ab.py [--config c2] [--k 96] [--budget MiB[,MiB...]] [--steps 3]
                                 [--warmup 1] [--reps 2] [--scale S] [--nz N] [--no-hash]

--k 128, 112, 97 run configuration c4 unless --config names another; its whole grid's factors
(313 GB) fit no single device, so --nz cuts the grid to its lowest N levels (--nz 25: 2.25 M
points, 157 GB of factors).
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

# by KP: the option (by number: an older abi.py has no name for it), the factor's bytes
# (BigFactor<96, 32>, BigFactor<128, 64>) and the kernels' names
BIG_REUSE, FACTOR_BYTES = 21, 8 * 4977
HIT = "solve_tqb_factor_kernel<96, 32>"
PAIR = ("solve_tq_big_kernel<96, false, 32>", "solve_tqb_tail_kernel<96, 32, 2>")
FILL_PAIR = ("(fill) solve_tq_big_kernel<96, false, 32>", "(fill) fill_tqb_tail_kernel<96, 32>")


def pick(k):
    global BIG_REUSE, FACTOR_BYTES, HIT, PAIR, FILL_PAIR
    if k > 96:
        BIG_REUSE, FACTOR_BYTES = 22, 8 * 8705
        HIT = "solve_tqb_factor_kernel<128, 64>"
        PAIR = ("solve_tq_rows_kernel<128, 64>", "solve_tqb_tail_kernel<128, 64, 3>")
        FILL_PAIR = ("(fill) solve_tq_rows_kernel<128, 64>", "(fill) fill_tqb_tail_kernel<128, 64>")


def has_option(k):
    c = abi.Core(k, device=0)
    try:
        c.set_option(BIG_REUSE, 1)
        return True
    except abi.CwblError:
        return False
    finally:
        c.finalize()


def measure(w, mode, budget, steps, warmup, reps, hashes):
    """None when mode is `on` and the cache holds nothing under `budget` (allocation failed)."""
    import torch
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
    var = to_dev(w.var)
    torch.cuda.synchronize()
    core = abi.Core(w.k, device=0)
    if mode == "on":
        core.set_option("record_reuse", budget)
        core.set_option(BIG_REUSE, 1)
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

    def digest():
        """SHA-256 of the analysis of the workload's own variable by the next call."""
        var.copy_(torch.from_numpy(w.var))
        timed()
        info = core.reuse_info().as_dict()
        return hashlib.sha256(var.cpu().numpy().tobytes()).hexdigest(), info

    core.set_obs(obs_set())
    for _ in range(max(1, warmup)):
        core.analyze_var(w.vp, slab)
    if mode == "on" and core.reuse_info().bytes_held == 0:
        core.finalize()
        return None
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
    core.set_kernel_timing(False)
    r["sha"] = []
    if mode == "on":  # the kernel times of a fill
        core.set_obs(obs_set())
        core.set_kernel_timing(True)
        fill = digest() if hashes else (timed(), None)[1]
        for name, t in core.kernel_times().items():
            r["kernels"]["(fill) " + name] = t
        core.set_kernel_timing(False)
        if hashes:
            r["sha"].append(("fill",) + fill)
            r["sha"].append(("hit",) + digest())
    elif hashes:
        r["sha"].append(("warm",) + digest())
    core.finalize()
    return r


def spread(v):
    return f"{np.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="c2 at k <= 96, c4 above")
    ap.add_argument("--k", type=int, default=96)
    ap.add_argument("--budget", default="200000,150000,100000,50000",
                    help="record_reuse in MiB: the first value whose cache allocation succeeds")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (trial runs)")
    ap.add_argument("--nz", type=int, default=None, help="cut the grid to its lowest NZ levels")
    ap.add_argument("--no-hash", action="store_true")
    args = ap.parse_args()
    pick(args.k)
    args.config = args.config or ("c4" if args.k > 96 else "c2")
    cut = {"nz": args.nz} if args.nz else {}
    w = synth.make(args.config, scale=args.scale, k=args.k, **cut)
    print(f"== {args.config}: {w.nx}x{w.ny}x{w.nz} grid, k={w.k}, {w.obs.shape[0]} obs"
          f"{' (scale %g)' % args.scale if args.scale else ''}"
          f"{' (nz cut to %d)' % args.nz if args.nz else ''}; steps={args.steps} "
          f"warmup={args.warmup} reps={args.reps}; library "
          f"{os.environ.get('CWBL_LIBRARY', '(this tree)')}", flush=True)
    modes = ("off", "on") if has_option(args.k) else ("off",)
    for mode in modes:
        r, budget = None, 0
        for budget in ([int(b) for b in args.budget.split(",")] if mode == "on" else [0]):
            r = measure(w, mode, budget, args.steps, args.warmup, args.reps, not args.no_hash)
            if r is not None:
                break
            print(f"on: record_reuse = {budget} MiB: nothing cached (allocation failed)")
        if r is None:
            continue
        both = [f + h for f, h in zip(r["first"], r["second"])]
        wi, fi = r["warm_info"], r["first_info"]
        print(f"{mode}:" + (f" record_reuse = {budget} MiB" if mode == "on" else ""))
        print(f"   warm ms per call    {spread(r['warm'])}   reused={wi['batches_reused']} "
              f"assembled={wi['batches_assembled']} held={wi['bytes_held'] / 2**30:.2f} GiB")
        print(f"   call after set_obs  {spread(r['first'])}   reused={fi['batches_reused']} "
              f"assembled={fi['batches_assembled']}")
        print(f"   call after it       {spread(r['second'])}")
        print(f"   sum of the two      {spread(both)}")
        kt = r["kernels"]
        for name, t in sorted(kt.items()):
            line = f"   {name:42s} {t['launches']:4d} launches {t['points']:9d} points {t['ms']:9.3f} ms"
            if name == HIT and t["ms"] > 0:
                # points with p = 0 read their info alone
                share = t["points"] / max(1, w.points)
                gb = r["solved"] * share * FACTOR_BYTES / 1e9
                line += f"   {gb:.1f} GB of factors at {gb / t['ms']:.2f} TB/s"
            print(line)
        # per 1000 points: what the acceptance line compares when not every batch is cached
        for label, names in (("head + tail", PAIR), ("head + fill tail", FILL_PAIR), ("hit", (HIT,))):
            if all(n in kt and kt[n]["points"] for n in names):
                per = sum(kt[n]["ms"] / kt[n]["points"] for n in names) * 1e3
                print(f"   {label:18s} {per:9.4f} ms per 1000 points")
        for what, sha, info in r["sha"]:
            print(f"   sha256 {what:5s} {sha}   reused={info['batches_reused']} "
                  f"assembled={info['batches_assembled']}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
