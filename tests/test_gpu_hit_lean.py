"""GPU tests of the merged hit kernel's lean text (solve_tq40_factor_merged_kernel, the LEAN
flag of tq40_factor_hit / tq40_factor_solve in cwbl_tq40_factor.h).

Under the flag the replay keeps each step's reflector where it found x, the back-transform
reads it from there, phase 2's columns and phase 1's prefix words are loaded without a per-lane
skip (the lanes above row j + 1 hold words of the column before, which the replay's select
masks), and T, qs and qz stand in LDS in the order the twisted walk takes them.  None of this
changes an operand of a floating-point expression, so every comparison here is exact: each
case makes one filling call and two hits under the default (merged) path and compares var bit
for bit (np.array_equal on the bit patterns) and the counters with the same calls under
hit_merge = 0 (solve_tq40_factor_kernel, which does not set the flag) and under
record_reuse = 0 (solve_tq40_kernel).  The per-point info is not exported by the ABI: the
counters are its reduction (solved, nobs_sum, sweeps_sum, max_sweeps, nonconverged), and
reuse_info shows that the calls taken for hits were hits.

The cases are the smallest shapes at which a piece of the lean text can go wrong: slabs of
720 to 833 points in batches of 256.
"""
import numpy as np
import pytest

import spectra_cases as sc
from cwbl import synth
from helpers import inflat_of, quad_level, radar_point_columns, spectrum_ratio

from reuse_harness import Inputs, Run, bits, is_hit, is_miss, no_reuse, other_var
from test_gpu_hit_merge import hit_launches

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL = {"max_batch": 256, "split40_batch": 128}


def small(**kw):
    """12 x 12 x 5 points, 120 obs: 720 points in batches of 256, 256 and 208."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, **kw)


def calls(inp, variables, merge, opts, host=False, hit_inp=None):
    """A fill on variables[0], then a hit on each of variables[0] and variables[1] under
    hit_merge = `merge` (hit_inp: the inputs of the hits, where their epilogue differs from the
    fill's): [(var, counters)] of the three calls and (launches, points) of the hit kernel."""
    o = dict(opts)
    o["hit_merge"] = merge
    r = Run(inp, opts=o, host=host)
    try:
        out, cnt, info = r.call(variables[0])
        is_miss(info)
        nbat = info["batches_assembled"]
        got = [(out, cnt)]
        if hit_inp is not None:
            r.sync(hit_inp)
        r.c.set_kernel_timing(True)
        for var in variables[:2]:
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            got.append((out, cnt))
        return got, hit_launches(r.c.kernel_times())
    finally:
        r.close()


def equal(a, b, what):
    assert a[1] == b[1], (what, a[1], b[1])
    assert np.array_equal(bits(a[0]), bits(b[0])), what


def check(inp, variables, opts=SMALL, host=False, hit_inp=None, windows=1, segments=None):
    """The merged hits against the per-batch hits and against no reuse.  Returns the no-reuse
    analyses of the two hits [(var, counters)]; segments: hit launches per call of the
    per-batch form."""
    fill_ref, = no_reuse(inp, variables[:1], opts=opts)
    want = no_reuse(hit_inp or inp, variables[:2], opts=opts)
    merged, (n1, p1) = calls(inp, variables, 1, opts, host, hit_inp)
    single, (n0, p0) = calls(inp, variables, 0, opts, host, hit_inp)
    points = want[0][1]["points"]
    # two hit calls: one merged launch per info window each, over every cached point
    assert (n1, p1) == (2 * windows, 2 * points), (n1, p1)
    assert p0 == 2 * points and n0 > n1, (n0, p0)
    assert segments is None or n0 == 2 * segments, n0
    equal(merged[0], fill_ref, "fill")
    for i in (0, 1):
        equal(merged[1 + i], single[1 + i], f"hit {i}: merged against hit_merge = 0")
        equal(merged[1 + i], want[i], f"hit {i}: merged against record_reuse = 0")
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    return want


@pytest.mark.parametrize("k", [40, 33, 24, 17])
def test_padding_rows(k):
    """k = 40 and the padded k = 33, 24, 17 on KP = 40: the rows past k of the reflectors the
    replay keeps, and of the walk-ordered T, are the padding's."""
    wl = small(k=k)
    want = check(Inputs(wl), [wl.var, other_var(wl, 3)])
    assert want[0][1]["points"] == 720 and want[0][1]["solved"] > 0


EPILOGUES = {"both": (1, 1, 0), "neither": (0, 0, 0), "rtpp": (1, 0, 0), "rtps_tune_q": (0, 1, 1)}


@pytest.mark.parametrize("name", sorted(EPILOGUES))
def test_epilogue_flags(name):
    """RTPP / RTPS on, off and mixed, tune_q once: the hits run under settings the fill did not
    have (the epilogue is no part of the cache's key)."""
    wl = small()
    inp, new = Inputs(wl), Inputs(wl)
    new.vp.use_rtpp, new.vp.use_rtps, new.vp.tune_q = EPILOGUES[name]
    new.vp.rtpp_alpha, new.vp.rtps_alpha = 0.5, 0.7
    want = check(inp, [wl.var, other_var(wl, 5)], hit_inp=new)
    old, = no_reuse(inp, [wl.var], opts=SMALL)
    assert not np.array_equal(bits(old[0]), bits(want[0][0]))


@pytest.mark.parametrize("sub,single", [(0, False), (50, True)])
def test_segments_and_staggered_slab(sub, single):
    """18 columns of which ix_lim = 17 are analysed, x 7 x 7 = 833 points, no multiple of four,
    in batches of 256, 256, 256 and 65: whole (four segments, the last one 65 points), and in
    sub-batches of 64 points, where the last batch gives a segment of 64 points and one of a
    single point.  The lanes past a segment read its spare record and aux entry."""
    wl = synth.make("c2", nx=18, ny=7, nz=7, n_obs=120)
    inp = Inputs(wl)
    inp.ix_lim = 17
    o = {"max_batch": 256, "split40_batch": sub}
    # the per-batch form has one launch per segment: 4 whole batches, or 4 + 4 + 4 + 2
    want = check(inp, [wl.var, other_var(wl, 5)], opts=o, segments=14 if single else 4)
    assert want[0][1]["points"] == 833


def test_sparse_obs():
    """Every 25th obs only (5 of 120): points with p = 1 .. 5 < k, whose steps past p have
    tau = 0 and scal = 0, so the kept reflector is e_(j+1).  The slab's columns i >= 8 stand
    1000 km away from every obs: their points have p = 0 and keep their bits."""
    wl = small()
    keep = np.arange(wl.obs.shape[0]) % 25 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    v2 = other_var(wl, 5)
    inp = Inputs(wl)
    inp.x[:, 8:] += np.float32(1e6)
    want = check(inp, [wl.var, v2])
    cnt = want[0][1]
    assert 0 < cnt["solved"] <= wl.points * 8 // 12 and cnt["max_p"] <= 5 < wl.k, cnt
    for (out, _), var in zip(want, (wl.var, v2)):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() >= wl.points - cnt["solved"]


# spectra_cases' record-path workloads at obs errors 2^-3, 2^-16 and, with 12 obs, 2^-6
SPECTRA = [c for c in sc.RECORD if (c.n_obs, c.e) in ((120, -3), (120, -16), (12, -6))]


@pytest.mark.parametrize("c", SPECTRA, ids=sc.case_id)
def test_wide_spectra(c):
    """test_gpu_analyze_vars_spectra.py's pair ensembles (k = 32) at obs errors 2^-3, 2^-16 and,
    with 12 obs (p = 3 .. 12 < k), 2^-6: levels above 3, 5 and 12, so the walk-ordered
    quadrature runs R = 2, 3, 4 and 8 rounds, two classes inside waves of four points."""
    assert sorted({r for s in SPECTRA for r in s.classes}) == [2, 3, 4, 8]
    wl = sc.workload(c)
    # every point's level from the fp64 spectrum bound, as spectra_cases.evaluate takes it
    infl = inflat_of(c.k, wl.vp.multi_infl)
    nz, ny, nx = wl.var.shape[1:]
    lv = np.zeros((nz, ny, nx), np.int32)
    for kz, j, i in np.ndindex(nz, ny, nx):
        yo, yb = radar_point_columns(wl, kz, j, i, 2.0 ** c.e)
        if len(yo):
            lv[kz, j, i] = quad_level(spectrum_ratio(yb, infl))
    assert sc.classes_present(c, lv) == sorted(c.classes)
    assert (sc.mixed_fours(c, lv) > 0) == c.mixed
    rng = np.random.default_rng(9)
    v2 = (wl.var + np.round(rng.standard_normal(wl.var.shape) * 64) / 64).astype(np.float32)
    want = check(Inputs(wl), [wl.var, v2])
    cnt = want[0][1]
    assert cnt["nonconverged"] == 0 and cnt["solved"] > 0, cnt
    print(f"{sc.case_id(c)}: levels {sorted(set(lv.ravel().tolist()) - {0})}")
    assert cnt["max_sweeps"] == lv.max() and cnt["solved"] == np.count_nonzero(lv), cnt


def test_non_finite_var():
    """NaN, +Inf and -Inf in single members of single points: the points' analyses carry the
    same non-finite bit patterns on every path, every other point its own bits."""
    wl = small()
    k = wl.k
    bad = wl.var.copy()
    flat = bad.reshape(k, -1)
    for n, g in enumerate((7, 130, 255, 256, 511)):
        flat[(3 * n) % k, g] = np.nan
    for n, g in enumerate((3, 257, 400)):
        flat[(5 * n + 1) % k, g] = np.inf
    for n, g in enumerate((64, 640, 719)):
        flat[(7 * n + 2) % k, g] = -np.inf
    want = check(Inputs(wl), [bad, wl.var])
    hit = np.any(~np.isfinite(want[0][0]), axis=0).ravel()
    assert hit[[7, 130, 255, 256, 511, 3, 257, 400, 64, 640, 719]].all() and hit.sum() == 11
    assert np.isfinite(want[1][0]).all()


def test_badly_scaled_obs():
    """Every obs scaled by its own power of two, 2^-12 .. 2^12 (value and ensemble alike, which
    is an obs error 2^12 .. 2^-12 times the type's): the factor's neighbouring words, which the
    plain loads bring into the masked lanes, differ by many orders of magnitude."""
    wl = small()
    rng = np.random.default_rng(17)
    s = (2.0 ** rng.integers(-12, 13, wl.obs.shape[0])).astype(np.float32)
    wl.obs = (wl.obs * s).astype(np.float32)
    wl.hdxb = np.ascontiguousarray((wl.hdxb * s[None, :]).astype(np.float32))
    inp = Inputs(wl)
    inp.tp.err_rej[0] = 1e9  # keep the scaled departures
    want = check(inp, [wl.var, other_var(wl, 5)])
    cnt = want[0][1]
    assert cnt["solved"] > 0 and cnt["max_sweeps"] >= 6, cnt
    assert np.isfinite(want[0][0]).all()
