"""What the GPU suites of the record cache and of the factor caches share (not a test module):
the inputs of a call, one library state, the analyses without reuse, the hit and miss checks
of cwbl_reuse_info, and the factor-cache suites' small workloads and invalidating changes.

Every comparison of analyses is exact (`same`: np.array_equal on the bit patterns, equality of
the counters).
"""
import copy
import functools

import numpy as np
import pytest

from cwbl import abi, synth

torch = pytest.importorskip("torch")

# the record-path suites' batches: search batches of 1024 points, record sub-batches of 512
OPTS = {"max_batch": 1024, "split40_batch": 512}
# the factor-cache suites': 720 points in batches of 256, 256 and 208
BATCH = {"max_batch": 256}
COUNTERS = ("points", "solved", "nobs_sum", "lz_truncated", "nonconverged", "q1_undefined",
            "sweeps_sum", "max_p", "max_sweeps", "ntrees")


def counters(st):
    return {n: getattr(st, n) for n in COUNTERS}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def other_var(w, seed):
    """Another variable on the same grid: the same shape, other values."""
    rng = np.random.default_rng(seed)
    return (w.var + rng.standard_normal(w.var.shape, dtype=np.float32)).astype(np.float32)


class Inputs:
    """Everything a call depends on but var; copied so that a test can change any of it."""

    def __init__(self, w):
        self.k, self.radar_type = w.k, w.radar_type
        self.x, self.y, self.alt = w.x.copy(), w.y.copy(), w.alt.copy()
        self.obs_xyz, self.obs, self.hdxb = w.obs_xyz, w.obs, w.hdxb
        self.vp = copy.deepcopy(w.vp)
        self.ix_lim = None
        self.options = {}

    @property
    def tp(self):
        return self.vp.radar[self.radar_type - 1]


class Run:
    """One library state: the slab's coordinates live in device buffers that stay where they
    are (sync() rewrites them in place), var is uploaded afresh for every call.  The options are
    `opts` over `base` (the record-path suites' OPTS unless given); `core`: cwbl_init's further
    arguments (weight_function)."""

    def __init__(self, inp, reuse=None, opts=None, host=False, base=OPTS, **core):
        options = dict(base)
        options.update(opts or {})
        if reuse is not None:
            options["record_reuse"] = reuse
        self.c = abi.Core(inp.k, device=0, options=options, **core)
        self.host = host
        self.inp = inp
        self.x, self.y, self.alt = (a.copy() if host else to_dev(a) for a in (inp.x, inp.y, inp.alt))
        self.hdxb = None
        self.applied = {}
        self.sync(inp)

    def sync(self, inp):
        self.inp = inp
        for dst, src in ((self.x, inp.x), (self.y, inp.y), (self.alt, inp.alt)):
            if self.host:
                dst[...] = src
            else:
                dst.copy_(torch.from_numpy(src))
        if inp.hdxb is not self.hdxb:
            self.c.set_obs(abi.ObsSetBuilder().add_radar(inp.radar_type, inp.obs_xyz, inp.obs,
                                                         inp.hdxb).build())
            self.hdxb = inp.hdxb
        for name, value in inp.options.items():
            if self.applied.get(name) != value:
                self.c.set_option(name, value)
                self.applied[name] = value

    def call(self, var):
        """Analyse a copy of `var`: (analysis, counters, reuse_info)."""
        inp = self.inp
        if self.host:
            v = np.array(var, np.float32, copy=True)
            slab = abi.make_slab(self.x, self.y, self.alt, v, ix_lim=inp.ix_lim)
        else:
            v = to_dev(var)
            torch.cuda.synchronize()
            slab = abi.make_slab(self.x, self.y, self.alt, v, ix_lim=inp.ix_lim,
                                 memory=abi.MEM_DEVICE)
        st = self.c.analyze_var(inp.vp, slab)
        out = v if self.host else v.cpu().numpy()
        return out, counters(st), self.c.reuse_info().as_dict()

    def close(self):
        self.c.finalize()


def _without_reuse(r, variables):
    try:
        outs = []
        for var in variables:
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 0 and info["bytes_held"] == 0, info
            outs.append((out, cnt))
        return outs
    finally:
        r.close()


def no_reuse(inp, variables, opts=None):
    """The analyses of `variables` with record_reuse = 0, one after the other."""
    return _without_reuse(Run(inp, reuse=0, opts=opts), variables)


def off(inp, variables, opts=None, **core):
    """The analyses of `variables` in batches of 256 with record_reuse = 0 and the factor caches'
    options at their default 0: [(out, counters)]."""
    if not core:
        return no_reuse(inp, variables, opts=dict(BATCH, **(opts or {})))
    return _without_reuse(Run(inp, reuse=0, opts=dict(BATCH, **(opts or {})), base={}, **core),
                          variables)


def is_miss(info, nbat=None, several=True):
    """Nothing reused; `several`: more than one batch assembled (the record-path suites'
    workloads all have several); nbat: exactly that many."""
    assert info["batches_reused"] == 0, info
    assert not several or info["batches_assembled"] > 1, info
    assert nbat is None or info["batches_assembled"] == nbat, info


def is_hit(info, nbat):
    assert info["batches_reused"] == nbat and info["batches_assembled"] == 0, info
    assert info["bytes_held"] > 0, info


def same(got, want):
    assert got[1] == want[1], (got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))


# ---- the factor-cache suites' workloads ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small(k):
    """12 x 12 x 5 points, 120 obs: 720 points, batches of 256, 256 and 208."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)


@functools.lru_cache(maxsize=None)
def small_refs(k):
    """The analyses of small(k)'s var and of two other variables with the option off; shared,
    never modified."""
    w = small(k)
    return no_reuse(Inputs(w), [w.var, other_var(w, 5), other_var(w, 6)], opts=BATCH)


def sparse(k, every=40):
    wl = copy.copy(small(k))
    keep = np.arange(wl.obs.shape[0]) % every == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    return wl


@functools.lru_cache(maxsize=None)
def ragged(k):
    """A 14 x 11 x 5 slab: 715 points under ix_lim = 13."""
    return synth.make("c2", seed=11, nx=14, ny=11, nz=5, n_obs=120, k=k)


# ---- changes of one input of a cached factor ----------------------------------------------------
def _x_in_place(inp, w):
    inp.x += np.float32(500.0)


def _set_obs(inp, w):
    rng = np.random.default_rng(5)
    inp.hdxb = (w.hdxb + rng.standard_normal(w.hdxb.shape, dtype=np.float32)).astype(np.float32)


def _hclr(inp, w):
    inp.tp.hclr = 10.0


def _multi_infl(inp, w):
    inp.vp.multi_infl = 1.1


CHANGES = {"x_in_place": _x_in_place, "set_obs": _set_obs, "hclr": _hclr,
           "multi_infl": _multi_infl}
