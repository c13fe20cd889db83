"""GPU tests of the merged hit kernel's level from the kept info (solve_tq40_factor_merged_kernel,
the LEAN flag of tq40_factor_solve in cwbl_tq40_factor.h).

A solved point's quadrature level is no longer worked out from trace(T) on a hit: the kernel
takes the +-level that the fill's solve stored in the point's info, which the cache keeps, and
stores that word again.  The lanes that have none (a point with p = 0, a lane past its segment)
still sum their record's trace, whatever that record holds, and compare it with the three traces
at which the wave's rounds change (hit_level_cuts, on the host); only waves with such a lane do.
Nothing of it changes an operand of a floating-point expression, so every comparison is exact:
a fill and two hits under the default (merged) path against the same calls under hit_merge = 0
(solve_tq40_factor_kernel, which keeps the trace, the division and the decade loop) and under
record_reuse = 0 (solve_tq40_kernel): np.array_equal on var's bit patterns and equal counters.
The per-point info is not exported by the ABI; the counters are its reduction (solved,
nobs_sum, sweeps_sum, max_sweeps = the highest level, nonconverged = the negative ones), taken
from the info that the hit stored.

Slabs of 4 to 720 points in batches of 256, at k = 40 and k = 33 (k = 32 where the ensemble
has to be one of member pairs).
"""
import numpy as np
import pytest

from cwbl import abi, synth
from helpers import (inflat_of, pair_ensemble, quad_level, quad_rounds, radar_point_columns,
                     spectrum_ratio)

from reuse_harness import Inputs, Run, bits, no_reuse, other_var
from test_gpu_hit_merge import hit_launches

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL = {"max_batch": 256, "split40_batch": 128}
KS = [40, 33]


def calls(inp, variables, merge, opts, host=False, hit_inp=None):
    """A fill on variables[0], then a hit on each of variables[0] and variables[1] under
    hit_merge = `merge` (hit_inp: the hits' inputs, where their epilogue is not the fill's):
    [(var, counters)] of the three calls, (launches, points) of the hit kernel."""
    o = dict(opts)
    o["hit_merge"] = merge
    r = Run(inp, opts=o, host=host)
    try:
        out, cnt, info = r.call(variables[0])
        assert info["batches_reused"] == 0 and info["batches_assembled"] > 0, info
        nbat = info["batches_assembled"]
        got = [(out, cnt)]
        if hit_inp is not None:
            r.sync(hit_inp)
        r.c.set_kernel_timing(True)
        for var in variables[:2]:
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == nbat and info["batches_assembled"] == 0, info
            got.append((out, cnt))
        return got, hit_launches(r.c.kernel_times())
    finally:
        r.close()


def equal(a, b, what):
    assert a[1] == b[1], (what, a[1], b[1])
    assert np.array_equal(bits(a[0]), bits(b[0])), what


def check(inp, variables, opts=SMALL, host=False, hit_inp=None, windows=1):
    """The merged hits against the per-batch hits and against no reuse; returns the no-reuse
    analyses of the two hits [(var, counters)]."""
    fill_ref, = no_reuse(inp, variables[:1], opts=opts)
    want = no_reuse(hit_inp or inp, variables[:2], opts=opts)
    merged, (n1, p1) = calls(inp, variables, 1, opts, host, hit_inp)
    single, (n0, p0) = calls(inp, variables, 0, opts, host, hit_inp)
    points = want[0][1]["points"]
    # two hit calls: one merged launch per info window each, over every cached point
    assert (n1, p1) == (2 * windows, 2 * points), (n1, p1)
    assert p0 == 2 * points and n0 >= n1, (n0, p0)
    equal(merged[0], fill_ref, "fill")
    for i in (0, 1):
        equal(merged[1 + i], single[1 + i], f"hit {i}: merged against hit_merge = 0")
        equal(merged[1 + i], want[i], f"hit {i}: merged against record_reuse = 0")
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    return want


def small(**kw):
    """12 x 12 x 5 points, 120 obs: 720 points in batches of 256, 256 and 208."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, **kw)


def fours(mask):
    """The aligned groups of four consecutive points (the waves: every batch starts at a
    multiple of four; the slab's last points, where they are no full group, left out) in which
    some points but not all have `mask`."""
    n = mask[:mask.size // 4 * 4].reshape(-1, 4).sum(axis=1)
    return int(np.count_nonzero((n > 0) & (n < 4)))


@pytest.mark.parametrize("k", KS)
def test_lanes_past_the_segment(k):
    """13 x 11 columns (ix_lim) x 5 levels = 715 points in batches of 256, 256 and 203, whole
    and in sub-batches of 64 points (the last one 11): the last wave of a ragged segment has
    lanes past it, which read the spare record and feed the ballot of the wave's rounds."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120, k=k)
    inp = Inputs(wl)
    inp.ix_lim = 13
    for sub in (0, 50):
        want = check(inp, [wl.var, other_var(wl, 5)], opts={"max_batch": 256, "split40_batch": sub})
        assert want[0][1]["points"] == 715 and want[0][1]["solved"] > 0


@pytest.mark.parametrize("k", KS)
def test_unsolved_points_inside_waves(k):
    """Every 25th obs only, and the slab's columns i >= 6 a thousand km from every obs: their
    points have p = 0, info (0, 0) and a record that no assembly wrote, and the waves of points
    i = 4 .. 7 hold solved points beside them."""
    wl = small(k=k)
    keep = np.arange(wl.obs.shape[0]) % 25 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    v2 = other_var(wl, 5)
    inp = Inputs(wl)
    inp.x[:, 6:] += np.float32(1e6)
    want = check(inp, [wl.var, v2])
    cnt = want[0][1]
    assert 0 < cnt["solved"] <= wl.points // 2, cnt
    untouched = np.all(bits(want[0][0]) == bits(wl.var), axis=0)
    assert untouched.sum() >= wl.points - cnt["solved"]
    assert fours(untouched.ravel()) > 0


def scattered(k, e):
    """12 x 12 x 5 points, 12 obs at obs error 2^e, the points' positions shuffled over the slab
    (x and y over the columns, alt over all points), so that the four points of a wave are no
    neighbours and their levels differ.  k even: helpers.pair_ensemble's values."""
    wl = synth.make("c2", nx=12, ny=12, nz=5, n_obs=12, k=k)
    if k % 2 == 0:
        wl = pair_ensemble(wl, 2.0 ** e)
    else:
        cfg = wl.extra["cfg"]
        wl.vp = synth.radar_var_params(cfg["hclr"], cfg["vclr"], cfg["max_lz"], 2.0 ** e,
                                       cfg["err_rej"], wl.radar_type)
    p = np.random.default_rng(3).permutation(wl.x.size)
    wl.x = np.ascontiguousarray(wl.x.ravel()[p].reshape(wl.x.shape))
    wl.y = np.ascontiguousarray(wl.y.ravel()[p].reshape(wl.y.shape))
    p3 = np.random.default_rng(4).permutation(wl.alt.size)
    wl.alt = np.ascontiguousarray(wl.alt.ravel()[p3].reshape(wl.alt.shape))
    return wl


def level_map(wl, e):
    """Every point's level from the fp64 spectrum bound (0: p = 0), as spectra_cases.evaluate
    takes it."""
    infl = inflat_of(wl.k, wl.vp.multi_infl)
    nz, ny, nx = wl.var.shape[1:]
    lv = np.zeros((nz, ny, nx), np.int32)
    for kz, j, i in np.ndindex(nz, ny, nx):
        yo, yb = radar_point_columns(wl, kz, j, i, 2.0 ** e)
        if len(yo):
            lv[kz, j, i] = quad_level(spectrum_ratio(yb, infl))
    return lv


@pytest.mark.parametrize("k,e", [(40, -1.25), (40, -3.0), (33, -1.25), (33, -3.0)])
def test_levels_mixed_in_a_wave(k, e):
    """Obs error 2^-1.25: levels 1, 2 and 3 inside single waves (all R = 2: the kept level picks
    each point's own table).  2^-3: levels 2 .. 4, waves that mix R = 2 and R = 3, which the
    ballot takes from the kept levels."""
    wl = scattered(k, e)
    lv = level_map(wl, e)
    rows = lv.reshape(-1, 4)
    if e == -1.25:
        assert sum({1, 2, 3} <= set(r.tolist()) for r in rows) >= 20
    else:
        assert lv.max() >= 4
        assert sum(len({quad_rounds(int(v)) for v in r if v > 0}) > 1 for r in rows) >= 20
    rng = np.random.default_rng(9)
    v2 = (wl.var + np.round(rng.standard_normal(wl.var.shape) * 64) / 64).astype(np.float32)
    want = check(Inputs(wl), [wl.var, v2])
    cnt = want[0][1]
    print(f"k={k} e={e}: levels {np.bincount(lv.ravel()).tolist()}, counters {cnt}")
    assert cnt["nonconverged"] == 0 and cnt["solved"] == np.count_nonzero(lv), cnt
    assert cnt["max_sweeps"] == lv.max(), cnt


@pytest.mark.parametrize("k", [40, 32])
def test_spectrum_beyond_the_last_table(k):
    """test_gpu_analyze_vars_spectra.block_workload: M/m > 1e24 at the one analysed point, whose
    kept info.y is -24, in a wave with three points of p = 0.  Every call reports the negative
    level (nonconverged = 1, max_sweeps = 24): the hit stores the kept word."""
    from test_gpu_analyze_vars_spectra import block_workload
    wl, _, _ = block_workload(k, 46, 32)
    for rtpp, rtps in ((0, 0), (1, 1)):
        inp = Inputs(wl)
        inp.vp.use_rtpp, inp.vp.rtpp_alpha = rtpp, 0.9
        inp.vp.use_rtps, inp.vp.rtps_alpha = rtps, 0.7
        want = check(inp, wl.vars)
        for _, cnt in want:
            assert cnt["solved"] == 1 and cnt["nonconverged"] == 1 and cnt["max_sweeps"] == 24, cnt


@pytest.mark.parametrize("k", KS)
def test_nan_records(k, monkeypatch):
    """weight_function = 1 (test_gpu_factor_scalars.py's Gaspari-Cohn workload): some points'
    records, factors and traces are NaN.  Their kept level is the loop's for a NaN ratio, 1."""
    core = abi.Core
    monkeypatch.setattr(abi, "Core", lambda *a, **kw: core(*a, weight_function=1, **kw))
    wl = synth.make("c2", nx=13, ny=11, nz=5, k=k, vclr=-1.0, hclr=6.0, n_obs=300)
    want = check(Inputs(wl), [wl.var, other_var(wl, 3)])
    nan = np.isnan(want[0][0]).any(axis=0)
    assert 0 < nan.sum() < wl.points
    assert fours(nan.ravel()) > 0


@pytest.mark.parametrize("k", KS)
def test_info_windows(k):
    """info_window = 256 on 715 points: three windows, each restored from the kept info before
    its merged launch and reduced after it."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120, k=k)
    inp = Inputs(wl)
    inp.ix_lim = 13
    o = {"max_batch": 256, "split40_batch": 128, "info_window": 256}
    want = check(inp, [wl.var, other_var(wl, 5)], opts=o, windows=3)
    assert want[0][1]["points"] == 715


@pytest.mark.parametrize("k", KS)
def test_host_slab_staged_whole(k):
    """A host slab with ix_lim < nx is staged whole, so its hits are merged."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120, k=k)
    inp = Inputs(wl)
    inp.ix_lim = 13
    check(inp, [wl.var, other_var(wl, 5)], host=True)


EPILOGUES = {"both": (1, 1), "neither": (0, 0), "rtpp": (1, 0), "rtps": (0, 1)}


@pytest.mark.parametrize("name", sorted(EPILOGUES))
def test_epilogue_flags(name):
    """RTPP / RTPS on and off on the hits, whatever the fill had (the epilogue is no part of
    the cache's key, the level is none of the epilogue's)."""
    wl = small(k=33)
    inp, new = Inputs(wl), Inputs(wl)
    new.vp.use_rtpp, new.vp.use_rtps = EPILOGUES[name]
    new.vp.rtpp_alpha, new.vp.rtps_alpha = 0.5, 0.7
    check(inp, [wl.var, other_var(wl, 5)], hit_inp=new)
