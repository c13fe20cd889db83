#!/usr/bin/env python
"""Cold and warm cwbl_analyze_var per search-index mode (CWBL_OPT_INDEX, and mode 1 with the
columns numbered in the bins' cell order, CWBL_OPT_INDEX_ORDER = 1: the lines "1+o") at full-size
C2 and C5.

cold: a fresh cwbl_set_obs (which drops every cached index) plus the first cwbl_analyze_var,
      which builds the index: mode 0 the k-d tree and the bins on the host, mode 1 the bins on
      the device with the tree left to a host thread.
warm: the following calls, whose index comes from the cache.
Obs set and slab are in device memory, as in bench.py's headline.  Each mode gets its own
library state; one untimed set_obs + analyze_var first loads the kernels and sizes the
buffers.  Per mode the cwbl_prep_info split of the cold call is printed with the table.

  python scripts/index_cold.py [--configs c2 c5] [--reps 3] [--warm 3] [--scale S]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402


#: (label, options) per measured mode, in the order of the table
MODES = ((0, {"index": 0}), (1, {"index": 1}), ("1+o", {"index": 1, "index_order": 1}))


def measure(w, options, reps, warm):
    import torch
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt = to_dev(w.x), to_dev(w.y), to_dev(w.alt)
    var0 = to_dev(w.var)
    var = var0.clone()
    torch.cuda.synchronize()
    core = abi.Core(w.k, device=0, options=options)
    slab = abi.make_slab(x, y, alt, var, memory=abi.MEM_DEVICE)

    def obs_set():
        return abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(w.radar_type, oxyz, obs, hdxb).build()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    core.set_obs(obs_set())
    core.analyze_var(w.vp, slab)  # untimed: kernels loaded, buffers sized
    rows = []
    for _ in range(reps):
        var.copy_(var0)
        ms_set, _ = timed(lambda: core.set_obs(obs_set()))
        ms_first, st = timed(lambda: core.analyze_var(w.vp, slab))
        info = core.prep_info().as_dict()
        warm_ms = []
        for _ in range(warm):
            var.copy_(var0)
            ms, stw = timed(lambda: core.analyze_var(w.vp, slab))
            warm_ms.append(ms)
        winfo = core.prep_info().as_dict()
        rows.append(dict(ms_set=ms_set, ms_first=ms_first, warm=warm_ms, info=info, winfo=winfo,
                         ms_prep=st.ms_prep, ms_prep_warm=stw.ms_prep, solved=st.solved,
                         nobs_sum=st.nobs_sum, lz_truncated=st.lz_truncated,
                         ms_search=stw.ms_search, ms_solve=stw.ms_solve))
    # one more warm call with per-kernel HIP-event timing (not part of the table above)
    core.set_kernel_timing(True)
    var.copy_(var0)
    core.analyze_var(w.vp, slab)
    kt = core.kernel_times()
    core.set_kernel_timing(False)
    core.finalize()
    return rows, kt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c5"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (trial runs)")
    args = ap.parse_args()
    for name in args.configs:
        w = synth.make(name, scale=args.scale)
        print(f"== {name}: {w.nx}x{w.ny}x{w.nz} grid, k={w.k}, {w.obs.shape[0]} obs"
              f"{' (scale %g)' % args.scale if args.scale else ''}", flush=True)
        print("mode  set_obs ms  first ms   cold ms   warm ms  cold/warm  first/warm   "
              "ms_prep cold / warm")
        best = {}
        for mode, options in MODES:
            rows, kt = measure(w, options, args.reps, args.warm)
            for r in rows:
                wm = float(np.median(r["warm"]))
                cold = r["ms_set"] + r["ms_first"]
                print(f"{mode:>4}  {r['ms_set']:10.2f} {r['ms_first']:9.2f} {cold:9.2f} {wm:9.2f} "
                      f"{cold / wm:10.3f} {r['ms_first'] / wm:11.3f}   {r['ms_prep']:8.2f} / "
                      f"{r['ms_prep_warm']:.2f}", flush=True)
            r = min(rows, key=lambda q: q["ms_first"])
            best[mode] = r
            i = r["info"]
            print(f"      prep_info of the fastest cold call: trees_built={i['trees_built']} "
                  f"bins_built={i['bins_built']} bins_on_device={i['bins_on_device']} "
                  f"flagged_batches={i['flagged_batches']} ms_tree={i['ms_tree']:.2f} "
                  f"ms_bins={i['ms_bins']:.2f} ms_columns={i['ms_columns']:.2f} "
                  f"ms_tree_wait={i['ms_tree_wait']:.2f}")
            print(f"      warm call: bins_built={r['winfo']['bins_built']} "
                  f"ms_columns={r['winfo']['ms_columns']:.2f}; solved={r['solved']} "
                  f"nobs_sum={r['nobs_sum']} lz_truncated={r['lz_truncated']}", flush=True)
            print(f"      warm call, summed kernel time: search {r['ms_search']:.2f} ms, solve "
                  f"{r['ms_solve']:.2f} ms; per kernel (event-timed call): "
                  + ", ".join(f"{n.split('<')[0]} {v['ms']:.2f}" for n, v in kt.items()), flush=True)
        for key in ("solved", "nobs_sum", "lz_truncated"):
            assert best[0][key] == best[1][key] == best["1+o"][key], (key, best)
        f0, f1, fo = (best[m]["ms_first"] for m, _ in MODES)
        w0, w1, wo = (float(np.median(best[m]["warm"])) for m, _ in MODES)
        print(f"   first call, mode 1 against mode 0: {f1:.2f} / {f0:.2f} ms = {f1 / f0:.3f}; "
              f"warm: {w1:.2f} / {w0:.2f} ms = {w1 / w0:.3f}", flush=True)
        print(f"   first call, mode 1 in cell order against mode 0: {fo:.2f} / {f0:.2f} ms = "
              f"{fo / f0:.3f}; warm: {wo:.2f} / {w0:.2f} ms = {wo / w0:.3f} "
              f"(against mode 1: {wo / w1:.3f})\n", flush=True)


if __name__ == "__main__":
    main()
