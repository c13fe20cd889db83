"""GPU tests of the cache hit's instruction schedule (solve_tq40_factor_kernel: the background
gathers issued with the factor's stream, the factor's loads in the order of their first use,
the walk's rows read one ahead).

None of it changes a floating-point expression, so every comparison is exact: np.array_equal
on the bit patterns and equal counters, against the analysis with record_reuse = 0, which
runs solve_tq40_kernel on freshly assembled records.  The fill kernel runs the same solve text
and is compared the same way.

Workloads: at most 13 x 11 x 5 points in batches of 256 and record sub-batches of 128 (or the
seams a test names), so that every launch has several waves and a ragged last one.
"""
import copy

import numpy as np
import pytest

from cwbl import synth

import spectra_cases as sc
from reuse_harness import (Inputs, Run, bits, is_hit, is_miss, no_reuse, other_var, same)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL = {"max_batch": 256, "split40_batch": 128}

#: (use_rtpp, use_rtps, tune_q): the four epilogues, and tune_q on one of them
EPILOGUES = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)]


def with_epilogue(inp, rtpp, rtps, tune_q):
    new = copy.copy(inp)
    new.vp = copy.deepcopy(inp.vp)
    new.vp.use_rtpp, new.vp.rtpp_alpha = rtpp, 0.9
    new.vp.use_rtps, new.vp.rtps_alpha = rtps, 0.7
    new.vp.tune_q = tune_q
    return new


def fill_then_two_hits(inp, variables, want, opts=SMALL, host=False, equal=same, one_batch=False):
    """A fill on variables[0], then a hit on each of variables[1:]; each equals `want`.
    (one_batch: the workload is a single batch, which is_miss does not take for a miss.)"""
    r = Run(inp, opts=opts, host=host)
    try:
        out, cnt, info = r.call(variables[0])
        if one_batch:
            assert info["batches_reused"] == 0 and info["batches_assembled"] == 1, info
        else:
            is_miss(info)
        nbat = info["batches_assembled"]
        equal((out, cnt), want[0])
        for var, ref in zip(variables[1:], want[1:]):
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            equal((out, cnt), ref)
    finally:
        r.close()


def three(wl):
    return [wl.var, other_var(wl, 5), other_var(wl, 6)]


def test_round_classes_of_the_cases():
    """The inputs' condition: R = 2, 3, 4 and 8 all occur across spectra_cases.RECORD, and at
    least one wave of four mixes two of them."""
    present, mixed = set(), 0
    for c in sc.RECORD:
        ev = sc.evaluate(c)
        here = sc.classes_present(c, ev.levels)
        assert here == sorted(c.classes), (sc.case_id(c), here)
        present |= set(here)
        mixed += sc.mixed_fours(c, ev.levels)
    assert present == {2, 3, 4, 8}, present
    assert mixed > 0


@pytest.mark.parametrize("c", sc.RECORD, ids=sc.case_id)
def test_every_round_class_with_every_epilogue(c):
    """A fill and two hits on other variables under each epilogue; the no-reuse run reports
    the levels that the case's classes were derived from."""
    wl = sc.workload(c)
    ev = sc.evaluate(c)
    variables = three(wl)
    for ep in EPILOGUES:
        inp = with_epilogue(Inputs(wl), *ep)
        want = no_reuse(inp, variables, opts=SMALL)
        assert want[0][1]["solved"] > 0 and want[0][1]["max_sweeps"] == ev.levels.max(), ep
        fill_then_two_hits(inp, variables, want)


def test_spectrum_beyond_the_last_table():
    """M/m > 1e24 at the one analysed point: level -24 from the fill and from both hits."""
    from test_gpu_analyze_vars_spectra import block_workload
    wl, _, _ = block_workload(32, 46, 32)
    for ep in ((0, 0, 0), (1, 1, 0)):
        inp = with_epilogue(Inputs(wl), *ep)
        want = no_reuse(inp, wl.vars, opts=SMALL)
        assert want[0][1]["nonconverged"] == 1 and want[0][1]["max_sweeps"] == 24
        fill_then_two_hits(inp, wl.vars, want, one_batch=True)


def sparse_715():
    """13 x 11 columns (ix_lim) x 5 levels = 715 points, no multiple of four; 120 obs with a
    horizontal localisation of 1 km, which reach 659 of the points (p <= 13) and leave 56 with
    p = 0 (the CPU oracle's count; asserted on the no-reuse run)."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120)
    inp = Inputs(wl)
    inp.tp.hclr = 1.0
    inp.ix_lim = 13
    return wl, inp


@pytest.mark.parametrize("sub", [37, 50])
def test_early_gathers_at_the_seams(sub):
    """Sub-batches of 37 and 50 points: the gathers of a wave's lanes past the launch and of
    the points with p = 0 are issued like every other lane's.  Those points' var holds NaN and
    Inf in some members and comes back untouched; the valid points equal no-reuse."""
    wl, inp = sparse_715()
    o = {"max_batch": 256, "split40_batch": sub}
    clean, = no_reuse(inp, [wl.var], opts=o)
    assert clean[1]["points"] == 715 and 0 < clean[1]["solved"] < 715, clean[1]
    # a point no obs reaches keeps every member's bits (the slab's last column is not analysed)
    kept = np.all(bits(clean[0]) == bits(wl.var), axis=0)
    kept[:, :, 13:] = False
    assert kept.sum() == 715 - clean[1]["solved"]
    variables = []
    for seed, bad in ((5, np.nan), (6, np.inf), (7, -np.inf)):
        v = other_var(wl, seed)
        v[3::7][:, kept] = bad
        v[1][kept] = np.nan
        variables.append(v)
    want = no_reuse(inp, variables, opts=o)
    for v, ref in zip(variables, want):
        assert ref[1] == clean[1]
        assert np.array_equal(bits(ref[0])[:, kept], bits(v)[:, kept])
        assert np.all(np.isfinite(ref[0][:, :, :, :13][:, ~kept[:, :, :13]]))
    fill_then_two_hits(inp, variables, want, opts=o)


def _u_like():
    wl = synth.make("c2", nx=13, ny=11, nz=5, n_obs=120)
    inp = Inputs(wl)
    inp.ix_lim = 12
    return wl, inp, {}


def _mu_like():
    wl = synth.make("c2", nx=13, ny=11, nz=1, n_obs=120)  # 143 points: one batch
    return wl, Inputs(wl), {"one_batch": True}


def _host():
    wl = synth.make("c2", nx=13, ny=11, nz=5, n_obs=120)
    return wl, Inputs(wl), {"host": True}


def _k17():
    wl = synth.make("c2", nx=13, ny=11, nz=5, n_obs=120, k=17)
    return wl, Inputs(wl), {}


def _k39():
    wl = synth.make("c2", nx=13, ny=11, nz=5, n_obs=120, k=39)
    return wl, Inputs(wl), {}


SLABS = {"ix_lim": _u_like, "nz1": _mu_like, "host": _host, "k17": _k17, "k39": _k39}


@pytest.mark.parametrize("shape", sorted(SLABS))
def test_slab_shapes_of_a_cycle_on_a_hit(shape):
    """One more column than ix_lim analyses (U-like), one level (MU-like), a host slab, and
    k = 17 and 39 (masked members): the gathers' addresses follow the slab's own strides."""
    wl, inp, kw = SLABS[shape]()
    variables = three(wl)
    want = no_reuse(inp, variables, opts=SMALL)
    assert want[0][1]["solved"] > 0
    fill_then_two_hits(inp, variables, want, **kw)


def nan_aware_same(got, want):
    """test_gpu_analyze_vars_spectra.nan_aware_equal, with the counters."""
    from test_gpu_analyze_vars_spectra import nan_aware_equal
    assert got[1] == want[1], (got[1], want[1])
    assert nan_aware_equal(got[0], want[0])


@pytest.mark.parametrize("ep", [(1, 1, 0), (0, 1, 0), (0, 0, 0)], ids=str)
def test_non_finite_variable_on_a_hit(ep):
    """NaN, +Inf and -Inf in one member at a few solved points, as a hit's variable and as the
    fill's: the bit patterns of no-reuse, NaNs at the same places."""
    wl = synth.make("c2", nx=13, ny=11, nz=5, n_obs=120)
    inp = with_epilogue(Inputs(wl), *ep)
    bad = other_var(wl, 5)
    flat = bad.reshape(wl.k, -1)
    for g, m, v in ((7, 3, np.nan), (130, 11, np.inf), (257, 0, -np.inf), (400, 39, np.nan),
                    (640, 8, np.inf), (714, 24, -np.inf)):
        flat[m, g] = v
    variables = [wl.var, bad, other_var(wl, 6)]
    want = no_reuse(inp, variables, opts=SMALL)
    assert want[0][1]["solved"] == wl.points  # the poisoned points are solved ones
    spoiled = ~np.all(np.isfinite(want[1][0]), axis=0)
    assert 6 <= spoiled.sum() < wl.points
    fill_then_two_hits(inp, variables, want, equal=nan_aware_same)
    fill_then_two_hits(inp, [bad, wl.var, bad], [want[1], want[0], want[1]],
                       equal=nan_aware_same)
