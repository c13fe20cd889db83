#!/usr/bin/env python
"""CWBL_OPT_HOST_PIPE against the whole-slab moves, from host memory, on the C2 grid at k = 40.

Cases (--cases):
  group1, group2, group4, group8   cwbl_analyze_vars of that many variables, record_reuse = 0
  tune_miss                        cwbl_analyze_var with tune_q = 1, record_reuse = 0
  tune_hit                         ... solved from the factor cache (filled by the untimed call)
  column                           cwbl_analyze_var under column_share = 1 with vclr = -1

Per case the modes below run alternating, --rounds times, in one process and session:

  dP   --parent's library (the parent commit's build), device slabs
  d0   this tree's library, device slabs, host_pipe = 0
  then for pageable numpy slabs ("pag") and page-locked ones ("pin", torch pin_memory):
  hP   the parent's library, host slabs
  h0   this tree's library, host slabs, host_pipe = 0
  h1   this tree's library, host slabs, host_pipe = 1

Per mode and round: one library state, cwbl_set_obs once (obs in device memory: the state of
a host's loop over its variables), one untimed call (it sizes every buffer, fills the cache of
tune_hit and gives the SHA-256 of the analyses, which must agree across all modes), then
--reps timed calls.  Every call starts from the pristine variables (restored untimed) and is
timed on the host clock around the call, which returns after its last copy.

Printed per case: median [min .. max] ms per mode, the SHA-256, transfer_info of this tree's
host modes, and the acceptance figures: |h0 - hP| against the session's run-to-run range, and
the host excess (host call minus the device-slab call of the same build) of h1 against hP's.

  python scripts/host_pipe_ab.py [--cases group8,tune_hit] [--reps 2] [--rounds 2]
                                 [--parent DIR/libcwbl.so] [--scale S] [--out FILE]
"""
import argparse
import copy
import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cwbnwp-letkf_amd"))

from cwbl import abi, synth  # noqa: E402

OUT = []
CASES = ("group1", "group2", "group4", "group8", "tune_miss", "tune_hit", "column")


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def q_like(shape, seed):
    """A moist-variable look-alike: N(1, 1) members, about one in six negative."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape, dtype=np.float32) + np.float32(1.0)


class Bench:
    """One workload's obs and coordinates on the device and on the host, and `nvar` pristine
    variables with a device copy, a pageable copy and a page-locked copy to analyse in."""

    def __init__(self, w, nvar, tune):
        import torch
        self.torch, self.w, self.nvar = torch, w, nvar
        dev = torch.device("cuda:0")
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.oxyz, self.obs, self.hdxb = to_dev(w.obs_xyz), to_dev(w.obs), to_dev(w.hdxb)
        self.dxyz = [to_dev(a) for a in (w.x, w.y, w.alt)]
        self.hxyz = [np.ascontiguousarray(a, np.float32) for a in (w.x, w.y, w.alt)]
        self.pristine = [q_like(w.var.shape, 700 + i) if tune else
                         (w.var if i == 0 else w.var + q_like(w.var.shape, 700 + i))
                         for i in range(nvar)]
        self.pristine = [np.ascontiguousarray(p, np.float32) for p in self.pristine]
        self.bufs = {"dev": [to_dev(p) for p in self.pristine],
                     "pag": [p.copy() for p in self.pristine]}
        self.keep = [torch.empty(p.shape, dtype=torch.float32).pin_memory() for p in self.pristine]
        self.bufs["pin"] = [t.numpy() for t in self.keep]
        self.vps = []
        for _ in range(nvar):
            vp = copy.deepcopy(w.vp)
            vp.tune_q = int(tune)
            self.vps.append(vp)
        torch.cuda.synchronize()

    def slabs(self, mem):
        if mem == "dev":
            return [abi.make_slab(*self.dxyz, b, memory=abi.MEM_DEVICE) for b in self.bufs[mem]]
        return [abi.make_slab(*self.hxyz, b) for b in self.bufs[mem]]

    def restore(self, mem):
        for b, p in zip(self.bufs[mem], self.pristine):
            if mem == "dev":
                b.copy_(self.torch.from_numpy(p))
            else:
                np.copyto(b, p)
        self.torch.cuda.synchronize()

    def digest(self, mem):
        h = hashlib.sha256()
        for b in self.bufs[mem]:
            h.update((b.cpu().numpy() if mem == "dev" else b).tobytes())
        return h.hexdigest()

    def run(self, lib, opts, mem, single, reps, ours):
        """-> (ms per timed call, SHA-256 of the untimed call's analyses, transfer_info or None)"""
        core = abi.Core(self.w.k, device=0, lib=lib, options=opts)
        core.set_obs(abi.ObsSetBuilder(abi.MEM_DEVICE).add_radar(
            self.w.radar_type, self.oxyz, self.obs, self.hdxb).build())
        slabs = self.slabs(mem)

        def rep():
            self.restore(mem)
            t0 = time.perf_counter()
            if single:
                core.analyze_var(self.vps[0], slabs[0])
            else:
                core.analyze_vars(self.vps, slabs)
            self.torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        rep()  # untimed: buffers sized, the cache filled
        sha = self.digest(mem)
        ms = [rep() for _ in range(reps)]
        info = core.transfer_info().as_dict() if ours and mem != "dev" else None
        core.finalize()
        return ms, sha, info


def stat(ms):
    return f"{np.median(ms):10.3f}  [{min(ms):.3f} .. {max(ms):.3f}]"


def load_parent(path, here):
    """The parent's library with the prototypes of the entry points it has (it lacks this
    change's)."""
    import ctypes
    parent = ctypes.CDLL(os.path.abspath(path))
    for name in abi.EXPORTS:
        if hasattr(parent, name):
            fn, ours = getattr(parent, name), getattr(here, name)
            fn.argtypes, fn.restype = ours.argtypes, ours.restype
    return parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="the parent commit's libcwbl.so (modes dP, hP)")
    ap.add_argument("--scale", type=float, default=None, help="shrink the grid (a quick look)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "host_pipe.txt"))
    args = ap.parse_args()
    here = abi.load_library()
    parent = load_parent(args.parent, here) if args.parent else None
    for case in args.cases.split(","):
        assert case in CASES, case
        nvar = int(case[5:]) if case.startswith("group") else 1
        tune, single = case.startswith("tune"), not case.startswith("group")
        base = {} if case == "tune_hit" else {"record_reuse": 0}
        over = {}
        if case == "column":
            base["column_share"] = 1
            over["vclr"] = -1.0
        w = synth.make("c2", k=40, scale=args.scale, **over)
        mb = w.var.nbytes / 1e6
        say(f"== {case}: c2 {w.nx}x{w.ny}x{w.nz} = {w.points} points, k={w.k}, "
            f"{w.obs.shape[0]} obs{' (scale %g)' % args.scale if args.scale else ''}; "
            f"{nvar} x {mb:.0f} MB of var each way; options {base}; reps={args.reps} x "
            f"rounds={args.rounds}; ms per call, median [min .. max]")
        b = Bench(w, nvar, tune)
        modes = []  # (name, library, options, memory)
        if parent:
            modes.append(("dP", parent, base, "dev"))
        modes.append(("d0", here, dict(base, host_pipe=0), "dev"))
        for mem in ("pag", "pin"):
            if parent:
                modes.append((f"hP {mem}", parent, base, mem))
            modes.append((f"h0 {mem}", here, dict(base, host_pipe=0), mem))
            modes.append((f"h1 {mem}", here, dict(base, host_pipe=1), mem))
        b.run(here, dict(base, host_pipe=0), "dev", single, 0, True)  # untimed: kernels loaded
        res = {m[0]: dict(ms=[], sha=None, info=None) for m in modes}
        for _ in range(args.rounds):
            for name, lib, opts, mem in modes:
                ms, sha, info = b.run(lib, opts, mem, single, args.reps, lib is here)
                r = res[name]
                r["ms"] += ms
                r["sha"], r["info"] = sha, info
        for name, _, _, _ in modes:
            r = res[name]
            say(f"   {name:7s}{stat(r['ms'])}   sha256 {r['sha']}")
            if r["info"]:
                say(f"          transfer_info {r['info']}")
        shas = {r["sha"] for r in res.values()}
        say(f"   analyses bit-equal across the modes: {len(shas) == 1}")
        med = {n: float(np.median(r["ms"])) for n, r in res.items()}
        for mem in ("pag", "pin"):
            if parent:
                p, z = res[f"hP {mem}"]["ms"], res[f"h0 {mem}"]["ms"]
                gap = abs(med[f"hP {mem}"] - med[f"h0 {mem}"])
                rng = max(max(p) - min(p), max(z) - min(z))
                say(f"   {mem}: |median hP - median h0| = {gap:.3f} ms, run-to-run range "
                    f"{rng:.3f} ms: {'within' if gap <= rng else 'NOT within'}")
            ref = "P" if parent else "0"
            ex_ref = med[f"h{ref} {mem}"] - med[f"d{ref}"]
            ex_1 = med[f"h1 {mem}"] - med["d0"]
            say(f"   {mem}: host excess h{ref} - d{ref} = {ex_ref:.3f} ms, h1 - d0 = {ex_1:.3f} ms: "
                f"ratio {ex_1 / ex_ref:.3f} ({'at most' if ex_1 <= 0.5 * ex_ref else 'NOT at most'} "
                f"half)")
        say()
        del b
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # (after every case: a later failure keeps what ran)
            f.write("\n".join(OUT) + "\n")
        assert len(shas) == 1, "the modes' analyses differ"


if __name__ == "__main__":
    main()
