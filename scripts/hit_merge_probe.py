#!/usr/bin/env python
"""The warm hit step as bench.py times it, for one build of the library and one set of options.

One run measures one library (CWBL_LIBRARY, or the tree's own).  Obs set and slab in device
memory, `--warmup` untimed calls, then `--reps` blocks of `--steps` calls, each block timed
between two device synchronisations (bench.py's timed region).  It prints one line, `PROBE` and
a JSON object: the options, what the last call reused, and the ms per step of every block.

  --max-batch N   CWBL_OPT_MAX_BATCH: a finer plan, i.e. more launches per hit step (the probe
                  of profiles/hit_merge.txt: the step against the number of launches)
  --hit-merge V   CWBL_OPT_HIT_MERGE (left at the library's default when not given, so that a
                  library without the option can be measured)

  python scripts/hit_merge_probe.py [--config c2] [--steps 20] [--warmup 5] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--max-batch", type=int, default=0)
    ap.add_argument("--hit-merge", type=int, default=-1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-timing", type=int, default=1, help="as bench.py: on")
    a = ap.parse_args()
    import torch
    w = synth.make(a.config)
    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    oxyz, obs, hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
    x, y, alt, var = to_dev(w.x), to_dev(w.y), to_dev(w.alt), to_dev(w.var)
    torch.cuda.synchronize()
    opts = {}
    if a.max_batch > 0:
        opts["max_batch"] = a.max_batch
    if a.hit_merge >= 0:
        opts["hit_merge"] = a.hit_merge
    core = abi.Core(w.k, device=0, options=opts or None)
    core.set_kernel_timing(bool(a.kernel_timing))
    slab = abi.make_slab(x, y, alt, var, memory=abi.MEM_DEVICE)
    core.set_obs(abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(w.radar_type, oxyz, obs, hdxb).build())
    for _ in range(a.warmup):
        core.analyze_var(w.vp, slab)
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            st = core.analyze_var(w.vp, slab)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    info = core.reuse_info().as_dict()
    out = {"library": os.environ.get("CWBL_LIBRARY", "(this tree)"), "config": a.config,
           "max_batch": a.max_batch, "hit_merge": a.hit_merge,
           "batches_reused": info["batches_reused"],
           "batches_assembled": info["batches_assembled"],
           "ms_per_step": [round(m, 4) for m in ms], "ms_solve_last": round(st.ms_solve, 4)}
    core.finalize()
    print("PROBE " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
