"""The GPU tests of the factor caches of k = 41..128, written once for three forms (FORMS; not a
test module: tests/test_gpu_wave_reuse.py, test_gpu_big_reuse.py and test_gpu_rows_reuse.py each
take their form's tests from here, so a test keeps its module, name and id):

  wave  CWBL_OPT_WAVE_REUSE, the one-wavefront path at k = 41..64: a cwbl_analyze_var call whose
        key misses runs fill_tq_wave_kernel<KP> (solve_tq_kernel<KP>'s analysis, which also
        leaves each point's factor A = Q T Q^T), and a call with an equal key and bit-equal
        coordinates runs solve_tq_wave_factor_kernel<KP> on the kept factors and nothing before it.
  big   CWBL_OPT_BIG_REUSE, the hand-off path at k = 65..96: a miss runs the hand-off kernel
        solve_tq_big_kernel<96, false, 32> unchanged and fill_tqb_tail_kernel<96, 32> in the
        place of solve_tqb_tail_kernel<96, 32, 2>; a hit runs solve_tqb_factor_kernel<96, 32> alone,
        once per sub-batch (CWBL_OPT_BIG_BATCH).
  rows  CWBL_OPT_ROWS_REUSE, the same at k = 97..128 behind the half-row hand-off kernel
        solve_tq_rows_kernel<128, 64>: the kernels at <128, 64>, the tail at <128, 64, 3>.

The fill is the plain kernel's text and the hit replays its x' expressions in its order, so every
comparison of analyses here is exact (np.array_equal on the bit patterns) and every comparison
of counters is equality, against the same inputs with the option off (record_reuse = 0 as
well: reuse_harness.off, no_reuse).

Workloads: 12 x 12 x 5 points with 120 obs in batches of 256, 256 and 208; 13 x 11 x 5 = 715
points (ix_lim < nx) for ragged ends.  Ensemble sizes: k = KP (no padding rows) and padded ones
(Form.ks; 65 and 97 have 31 padding rows and the shortest tail, 31 steps).  The quadrature has
two rules, 31 nodes (levels up to 12) and 63 nodes above: the spectra_cases of each form's
largest k hold both, each alone and mixed, and for wave block_workload(64, 46) the spectrum
beyond the last table.

A test reads what differs from its `form` (a fixture of the module that takes the test); `forms`
names the forms that have the test and `cases` its parameters per form; a form's module takes
all of it from suite_of.
"""
import collections
import ctypes as C
import dataclasses
import typing

import numpy as np
import pytest

import spectra_cases as sc
from cwbl import abi
from helpers import increment_rel_rms, oracle
from reuse_harness import (BATCH, CHANGES, Inputs, Run, bits, is_hit, is_miss, no_reuse, off,
                           other_var, ragged, same, small, small_refs, sparse, to_dev)

torch = pytest.importorskip("torch")

Names = collections.namedtuple("Names", "head plain fill hit")


def _sparse_wave(cnt, wl, k):
    """points with p = 0 and points with p < k (exactly-zero reflectors: the tau = 0 branch)"""
    assert 0 < cnt["solved"] < wl.points and cnt["nobs_sum"] / cnt["solved"] < k


def _sparse_handoff(cnt, wl, k):
    """three obs are left: points with p = 0, and points with p = 1 and p = 2, whose steps past
    the first ones are exactly-zero reflectors (tau = 0) in the hand-off kernel's half and in
    the tail's"""
    print(f"sparse k={k}: {cnt['solved']} points solved, {cnt['nobs_sum']} obs accepted, "
          f"max_p {cnt['max_p']}")
    # p <= 3 everywhere (three obs), some point with p >= 2 and some point with p < max_p
    assert 0 < cnt["solved"] < wl.points and 2 <= cnt["max_p"] <= 3
    assert cnt["solved"] < cnt["nobs_sum"] < cnt["max_p"] * cnt["solved"]


@dataclasses.dataclass(frozen=True)
class Form:
    id: str
    option: str
    ks: tuple             # k = KP first, then the padded sizes
    ks_ends: tuple        # truncated lists, NaNs, ragged points: KP and the most padded
    ks_budget: tuple      # test_partial_budget
    ks_host: tuple        # test_host_slab
    kp: typing.Callable   # the compiled KP of k
    head: typing.Optional[str]  # the hand-off kernel, which a fill runs unchanged
    plain: str            # what the fill kernel replaces ({kp}: KP)
    fill: str
    hit: str
    words: typing.Callable  # the exact fp64 words of a factor at KP
    bound_checked: bool   # words < the documented bound KP (KP - 1) / 2 + 5 KP, which then
                          # bounds bytes_held from above
    per_sub_batch: bool   # fills and hits are launched per sub-batch (CWBL_OPT_BIG_BATCH)
    spectra: tuple        # test_wide_spectra's cases
    inf_row: int          # test_nan_and_inf_members' Inf member (the NaN is in member 3)
    swapped: bool         # ... and a variable with the two swapped
    ignored: tuple        # accepted and ignored: (test id, k, further options, what runs)
    cache_names: tuple    # a kernel whose name holds one of these is a cache's
    sparse: typing.Callable  # what test_sparse_obs_and_untouched_points asserts of the counters

    @property
    def on(self):
        return {"max_batch": 256, self.option: 1}

    @property
    def top(self):
        return self.ks[0]

    def names(self, k):
        kp = self.kp(k)
        return Names(self.head, *(n.format(kp=kp) for n in (self.plain, self.fill, self.hit)))

    def bound(self, k):
        kp = self.kp(k)
        return kp * (kp - 1) // 2 + 5 * kp

    def cached(self, kt):
        return [n for n in kt if any(s in n for s in self.cache_names)]


WAVE = Form(
    id="wave", option="wave_reuse", ks=(64, 56, 48, 50), ks_ends=(64, 50), ks_budget=(64, 48),
    ks_host=(64, 48), kp=lambda k: (k + 7) // 8 * 8, head=None,
    plain="solve_tq_kernel<{kp}, false>", fill="fill_tq_wave_kernel<{kp}>",
    hit="solve_tq_wave_factor_kernel<{kp}>", words=lambda kp: kp * (kp - 1) // 2 + 5 * kp,
    bound_checked=False, per_sub_batch=False, spectra=tuple(c for c in sc.WAVE if c.k == 64),
    inf_row=11, swapped=False,
    ignored=(("16-more0", 16, {}, "solve_tq_kernel<16, false>"),  # k <= 16
             # k = 17..40 without the record split
             ("40-more1", 40, {"split40": 0}, "solve_tq_kernel<40, false>")),
    cache_names=("wave",), sparse=_sparse_wave)
BIG = Form(
    id="big", option="big_reuse", ks=(96, 80, 65), ks_ends=(96, 65), ks_budget=(96, 65),
    ks_host=(96, 80), kp=lambda k: 96, head="solve_tq_big_kernel<96, false, 32>",
    plain="solve_tqb_tail_kernel<96, 32, 2>", fill="fill_tqb_tail_kernel<96, 32>",
    hit="solve_tqb_factor_kernel<96, 32>", words=lambda kp: 4977,  # BigFactor<96, 32>
    bound_checked=True, per_sub_batch=True, spectra=tuple(c for c in sc.BIG if c.k == 96),
    inf_row=50, swapped=False,  # a member in each kernel's rows
    ignored=(("128-solve_tqb_tail_kernel<128, 64, 3>", 128, {},
              "solve_tqb_tail_kernel<128, 64, 3>"),  # k = 97..128
             ("64-solve_tq_kernel<64, false>", 64, {}, "solve_tq_kernel<64, false>")),  # k <= 64
    cache_names=("fill", "factor"), sparse=_sparse_handoff)
ROWS = Form(
    id="rows", option="rows_reuse", ks=(128, 112, 97), ks_ends=(128, 97), ks_budget=(128, 97),
    ks_host=(128, 112), kp=lambda k: 128, head="solve_tq_rows_kernel<128, 64>",
    plain="solve_tqb_tail_kernel<128, 64, 3>", fill="fill_tqb_tail_kernel<128, 64>",
    hit="solve_tqb_factor_kernel<128, 64>", words=lambda kp: 8705,  # BigFactor<128, 64>
    bound_checked=True, per_sub_batch=True, spectra=tuple(c for c in sc.BIG if c.k == 128),
    # one member in rows < 64 and one in rows >= 64: the two halves of the hand-off kernel's
    # v . x' sum
    inf_row=70, swapped=True,
    ignored=(("96-solve_tqb_tail_kernel<96, 32, 2>", 96, {},
              "solve_tqb_tail_kernel<96, 32, 2>"),  # k = 65..96
             ("64-solve_tq_kernel<64, false>", 64, {}, "solve_tq_kernel<64, false>")),  # k <= 64
    cache_names=("fill", "factor"), sparse=_sparse_handoff)
FORMS = (WAVE, BIG, ROWS)
HANDOFF = (BIG, ROWS)


def forms(*which):
    """The test belongs to these forms (to all, if none is named)."""
    def mark(fn):
        fn.forms = which or FORMS
        fn.cases = getattr(fn, "cases", [])
        return fn
    return mark


def cases(name, values, ids=None, which=FORMS):
    """... and runs once per value of values(form) as its argument `name` (the innermost
    decorator's values come first in the id)."""
    def mark(fn):
        fn.forms = which
        fn.cases = getattr(fn, "cases", []) + [(name, values, ids)]
        return fn
    return mark


def suite_of(form):
    """What a form's module puts into its namespace: the form's tests, the `form` fixture they
    take, and the hook that gives each test its cases."""
    @pytest.fixture(name="form")
    def fixture():
        return form

    def pytest_generate_tests(metafunc):
        for name, values, ids in getattr(metafunc.function, "cases", []):
            metafunc.parametrize(name, list(values(form)), ids=ids)

    names = {n: f for n, f in globals().items() if n.startswith("test_") and form in f.forms}
    return dict(names, form=fixture, pytest_generate_tests=pytest_generate_tests)


def run(form, inp, opts=None, **kw):
    """reuse_harness.Run with the form's option on, in batches of 256, and `opts`."""
    return Run(inp, opts=dict(form.on, **(opts or {})), base={}, **kw)


def miss(info, nbat=3):
    """A miss of exactly nbat batches (one, in test_spectrum_beyond_the_last_table)."""
    is_miss(info, nbat, several=False)


def fill_then_hits(form, inp, variables, want, nbat=3, nsub=1, opts=None, host=False,
                   points=None, **core):
    """A fill on variables[0], then a hit on every variable: each call equals `want` (the
    analyses with the option off, in order), counters included.  The fill ran the fill kernel
    (and the hand-off kernel, where the path has one) once per batch, or per sub-batch (nsub per
    batch), and neither the hit kernel nor the kernel the fill replaces; the hits ran the hit
    kernel over all `points`, as many launches per call, and neither a search, the hand-off
    kernel nor the plain kernel."""
    assert nsub == 1 or form.per_sub_batch
    n = form.names(inp.k)
    r = run(form, inp, opts, host=host, **core)
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(variables[0])
        miss(info, nbat)
        same((out, cnt), want[0])
        kt = r.c.kernel_times()
        assert n.fill in kt and n.hit not in kt and n.plain not in kt, kt
        assert kt[n.fill]["launches"] == nbat * nsub, kt
        if n.head:
            assert n.head in kt and kt[n.head]["launches"] == nbat * nsub, kt
        r.c.set_kernel_timing(True)
        for var, ref in zip(variables, want):
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert sorted(x for x in kt if x != "tune_q_kernel") == [n.hit], kt
        assert kt[n.hit]["launches"] == nbat * nsub * len(variables), kt
        if points is not None:
            assert kt[n.hit]["points"] == points * len(variables), kt
        return info
    finally:
        r.close()


# ---- fill and hit -----------------------------------------------------------------------------
@cases("k", lambda f: f.ks)
def test_fill_and_hits(form, k):
    """Fill with one variable, hit with it and with two others; the factor's bytes are held."""
    w = small(k)
    want = small_refs(k)
    assert want[0][1]["solved"] > 0 and want[0][1]["points"] == 720
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    info = fill_then_hits(form, Inputs(w), [w.var, other_var(w, 5), other_var(w, 6)], want,
                          points=720)
    # every batch's factors and its spare one, the accepted counts, the snapshot
    assert info["bytes_held"] >= (720 + 3) * form.words(form.kp(k)) * 8 + 8 * 720, info
    if form.bound_checked:
        assert info["bytes_held"] < (720 + 3) * form.bound(k) * 8 * (1 + 1 / 16) + (1 << 16), info


@cases("k", lambda f: f.ks, which=[f for f in FORMS if f.per_sub_batch])
def test_sub_batches(form, k):
    """big_batch = 128: every cached batch keeps two sub-batches' factors (128 + 128, 128 + 80),
    and a hit is one launch per sub-batch."""
    w = small(k)
    variables = [w.var, other_var(w, 5)]
    want = off(Inputs(w), variables, opts={"big_batch": 128})
    same(want[0], small_refs(k)[0])
    fill_then_hits(form, Inputs(w), variables, want, nsub=2, opts={"big_batch": 128}, points=720)


@cases("k", lambda f: f.ks)
def test_per_call_epilogue(form, k):
    """The hit call's RTPP / RTPS flags and alphas and tune_q, not the fill's."""
    w = small(k)
    inp, new = Inputs(w), Inputs(w)
    new.vp.use_rtpp, new.vp.rtpp_alpha = 0, 0.5
    new.vp.use_rtps, new.vp.rtps_alpha = 1, 0.7
    new.vp.tune_q = 1
    ref_new, = off(new, [w.var])
    assert not np.array_equal(bits(small_refs(k)[0][0]), bits(ref_new[0]))
    r = run(form, inp)
    try:
        out, cnt, info = r.call(w.var)
        miss(info)
        same((out, cnt), small_refs(k)[0])
        r.sync(new)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), ref_new)
        r.sync(inp)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), small_refs(k)[0])
    finally:
        r.close()


# ---- obs shapes -------------------------------------------------------------------------------
@cases("k", lambda f: f.ks)
def test_sparse_obs_and_untouched_points(form, k):
    """Every 40th obs: points with p = 0, which keep their input bits through the fill and the
    hits, and points with few obs (Form.sparse: what the form asserts of them)."""
    wl = sparse(k)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    cnt = want[0][1]
    form.sparse(cnt, wl, k)
    for (out, _), var in zip(want, variables):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() == wl.points - cnt["solved"]
    fill_then_hits(form, inp, variables, want)


@cases("k", lambda f: f.ks_ends)
def test_truncated_lists(form, k):
    """max_lz_pts = 6: every reached list truncates; a hit's counters come from the cache."""
    wl = small(k)
    inp = Inputs(wl)
    inp.tp.max_lz_pts = 6
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    assert want[0][1]["lz_truncated"] > 0
    fill_then_hits(form, inp, variables, want)


@cases("k", lambda f: f.ks_ends)
def test_gaspari_cohn_nans(form, k):
    """weight_function = 1: the reference's fp32 Gaspari-Cohn weights give NaN factors at some
    points; the hit reproduces the fill's NaNs bit for bit."""
    wl = small(k)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables, weight_function=1)
    assert not np.array_equal(bits(want[0][0]), bits(small_refs(k)[0][0]))
    print(f"gaspari-cohn k={k}: {int(np.isnan(want[0][0]).any(axis=0).sum())} NaN points")
    fill_then_hits(form, inp, variables, want, weight_function=1)


@cases("k", lambda f: f.ks_ends)
def test_nan_and_inf_members(form, k):
    """A variable with a NaN member (3) and an Inf member (Form.inf_row), as the fill's variable
    and as a hit's; where the form says so, also a hit's variable with the two swapped."""
    wl = small(k)
    inp = Inputs(wl)
    bad = wl.var.copy()
    bad[3, 2, 5, 7] = np.nan
    bad[form.inf_row, 4, 1, 2] = np.inf
    more = []
    if form.swapped:
        swap = wl.var.copy()
        swap[3, 2, 5, 7] = np.inf
        swap[form.inf_row, 4, 1, 2] = np.nan
        more = [swap]
    want_bad, *want_more = off(inp, [bad] + more)
    want_clean = small_refs(k)[0]
    for want in [want_bad] + want_more:
        finite = np.all(np.isfinite(want[0]), axis=0)
        assert 0 < finite.sum() < wl.points
    fill_then_hits(form, inp, [bad, wl.var] + more, [want_bad, want_clean] + want_more)
    fill_then_hits(form, inp, [wl.var, bad], [want_clean, want_bad])


# ---- quadrature rules -------------------------------------------------------------------------
@cases("c", lambda f: f.spectra, ids=sc.case_id)
def test_wide_spectra(form, c):
    """One pass (31 nodes), two (63 nodes), and both in one call: the hit takes its level from
    the trace of the factor's diagonal.  The levels against the CPU's level map."""
    from test_gpu_analyze_vars_spectra import check_levels
    wl = sc.workload(c)
    ev = sc.evaluate(c)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    present, mixed = check_levels(c, ev, want[0][1])
    print(f"{sc.case_id(c)}: passes {present}, {mixed} mixed fours")
    fill_then_hits(form, inp, variables, want)


@forms(WAVE)
def test_spectrum_beyond_the_last_table(form):
    """M/m > 1e24 at the one analysed point (three more with p = 0): level -24 from the fill
    and from the hit, counted in nonconverged both times."""
    from test_gpu_analyze_vars_spectra import block_workload
    wl, _, _ = block_workload(64, 46, 64)
    inp = Inputs(wl)
    want = off(inp, wl.vars)
    assert want[0][1]["nonconverged"] == 1 and want[0][1]["max_sweeps"] == 24
    fill_then_hits(form, inp, wl.vars, want, nbat=1)


# ---- slab kinds -------------------------------------------------------------------------------
@cases("host", lambda f: (False, True))
@cases("k", lambda f: f.ks_ends)
def test_ragged_points(form, k, host):
    """13 (ix_lim) x 11 x 5 = 715 points of a 14-column slab, batches of 256, 256 and 203; from
    device memory and from a pageable host slab."""
    wl = ragged(k)
    inp = Inputs(wl)
    inp.ix_lim = 13
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    assert want[0][1]["points"] == 715 and want[0][1]["solved"] > 0
    fill_then_hits(form, inp, variables, want, host=host, points=715)


@cases("k", lambda f: f.ks_host)
def test_host_slab(form, k):
    """A pageable host slab whose analysed region is the whole slab (var is piped batch by
    batch): fill, hits, and a miss after the caller rewrote alt in place."""
    w = small(k)
    want = small_refs(k)
    r = run(form, Inputs(w), host=True)
    try:
        fill = r.call(w.var)
        miss(fill[2])
        same(fill[:2], want[0])
        for var, ref in ((w.var, want[0]), (other_var(w, 5), want[1])):
            hit = r.call(var)
            is_hit(hit[2], 3)
            same(hit[:2], ref)
        r.alt += np.float32(37.0)
        miss(r.call(w.var)[2])
    finally:
        r.close()


@cases("window", lambda f: (256, 600))
def test_small_info_window(form, window):
    """One info window per batch (256) and a rollover inside the call (600): the hit restores
    the accepted counts window by window."""
    w = small(form.top)
    fill_then_hits(form, Inputs(w), [w.var, other_var(w, 5)], small_refs(form.top)[:2],
                   opts={"info_window": window})


@forms()
def test_device_built_index(form):
    """index = 1: a full hit needs neither the bins nor a tree."""
    w = small(form.top)
    inp = Inputs(w)
    variables = [w.var, other_var(w, 5)]
    want = off(inp, variables, opts={"index": 1})
    fill_then_hits(form, inp, variables, want, opts={"index": 1})


# ---- misses -----------------------------------------------------------------------------------
@cases("k", lambda f: f.ks_budget)
def test_partial_budget(form, k):
    """A budget that holds the first of three batches (257 factors) and not the second: later
    calls reuse that one, search and solve the other two with the path's own kernels."""
    w = small(k)
    per = form.words(form.kp(k)) * 8
    mib = (257 * per >> 20) + 1
    assert 257 * per <= mib << 20 < 2 * 257 * per
    want = small_refs(k)
    r = run(form, Inputs(w), reuse=mib)
    n = form.names(k)
    try:
        out, cnt, info = r.call(w.var)
        miss(info)
        assert 257 * per <= info["bytes_held"] < 2 * 257 * per
        same((out, cnt), want[0])
        r.c.set_kernel_timing(True)
        for var, ref in ((w.var, want[0]), (other_var(w, 5), want[1])):
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 1 and info["batches_assembled"] == 2, info
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert kt[n.hit]["points"] == 2 * 256 and kt[n.plain]["points"] == 2 * (720 - 256), kt
        assert n.fill not in kt, kt
        if n.head:
            assert kt[n.head]["points"] == 2 * (720 - 256), kt
    finally:
        r.close()


@forms()
def test_budget_of_zero_turns_the_cache_off(form):
    """... and on the hand-off path the plain tail runs, no cache kernel."""
    w = small(form.top)
    r = run(form, Inputs(w), reuse=0)
    n = form.names(form.top)
    try:
        if n.head:
            r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            miss(info)
            assert info["bytes_held"] == 0, info
            same((out, cnt), small_refs(form.top)[0])
        if n.head:
            kt = r.c.kernel_times()
            assert n.plain in kt and n.fill not in kt and n.hit not in kt, kt
    finally:
        r.close()


@cases("what", lambda f: sorted(CHANGES))
def test_invalidation(form, what):
    """After a fill and a hit one input of the factor changes (the obs set, a coordinate
    rewritten in place, a type parameter, multi_infl): a miss that equals the analysis of the new
    inputs with the option off, refilled over the old factors, then a hit again."""
    w = small(form.top)
    inp, new = Inputs(w), Inputs(w)
    CHANGES[what](new, w)
    ref_old = small_refs(form.top)[0]
    ref_new, = off(new, [w.var])
    assert not np.array_equal(bits(ref_old[0]), bits(ref_new[0]))
    r = run(form, inp)
    try:
        miss(r.call(w.var)[2])
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), ref_old)
        r.sync(new)
        out, cnt, info = r.call(w.var)
        miss(info)
        same((out, cnt), ref_new)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), ref_new)
    finally:
        r.close()


@forms(*HANDOFF)
def test_option_change_invalidates(form):
    """Any generation-bumping option voids the factors: big_batch changes the sub-batches."""
    w = small(form.top)
    want = small_refs(form.top)[0]
    r = run(form, Inputs(w))
    try:
        miss(r.call(w.var)[2])
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option("big_batch", 128)
        out, cnt, info = r.call(w.var)
        miss(info)
        same((out, cnt), want)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), want)
    finally:
        r.close()


# ---- calls that bypass the cache --------------------------------------------------------------
@forms()
def test_group_call_leaves_the_cache_valid(form):
    w = small(form.top)
    want = small_refs(form.top)
    r = run(form, Inputs(w))
    try:
        miss(r.call(w.var)[2])
        held = r.c.reuse_info().bytes_held
        bufs = [to_dev(w.var), to_dev(other_var(w, 5))]
        torch.cuda.synchronize()
        slabs = [abi.make_slab(r.x, r.y, r.alt, b, memory=abi.MEM_DEVICE) for b in bufs]
        r.c.analyze_vars([w.vp, w.vp], slabs)
        mid = r.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == held
        for b, ref in zip(bufs, want):
            assert np.array_equal(bits(b.cpu().numpy()), bits(ref[0]))
        out, cnt, info = r.call(other_var(w, 6))
        is_hit(info, 3)
        same((out, cnt), want[2])
    finally:
        r.close()


@forms()
def test_column_share_call_leaves_the_cache_valid(form):
    """test_gpu_column_share.test_cache_untouched at the form's largest k: a per-point call (a
    3-D type) fills, a column-shared call with other type parameters follows, the first call
    hits."""
    from test_gpu_analyze_vars import Lib
    from test_gpu_column_share import workload
    w3, w2 = workload(form.top, 9, "3d"), workload(form.top, 9, "dense")
    ref3, = no_reuse(Inputs(w3), [w3.var], opts=BATCH)
    lib = Lib(w3, dict(form.on, column_share=1), reuse_default=True)
    try:
        first, cnt = lib.one(w3.var, w3.vp)
        assert lib.c.column_info().reason == abi.COLUMN_REASON_3D
        fill = lib.c.reuse_info()
        assert fill.batches_assembled > 0 and fill.batches_reused == 0 and fill.bytes_held > 0
        assert cnt == ref3[1] and np.array_equal(bits(first), bits(ref3[0]))
        lib.one(w2.var, w2.vp)
        assert lib.c.column_info().shared == 1
        mid = lib.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == fill.bytes_held
        again, cnt2 = lib.one(w3.var, w3.vp)
        hit = lib.c.reuse_info()
        assert hit.batches_reused == fill.batches_assembled and hit.batches_assembled == 0
        assert cnt2 == cnt and np.array_equal(bits(again), bits(first))
    finally:
        lib.close()


# ---- option values ----------------------------------------------------------------------------
@forms()
def test_toggling_the_option_invalidates_and_releases(form):
    w = small(form.top)
    want = small_refs(form.top)[0]
    r = run(form, Inputs(w))
    n = form.names(form.top)
    try:
        miss(r.call(w.var)[2])
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option(form.option, 0)
        r.c.set_kernel_timing(True)
        for _ in range(2):  # option 0: nothing reused, nothing held, the path's own kernels
            out, cnt, info = r.call(w.var)
            miss(info)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert n.plain in kt and n.fill not in kt and n.hit not in kt, kt
        assert n.head in kt if n.head else not form.cached(kt), kt
        r.c.set_option(form.option, 1)
        miss(r.call(w.var)[2])
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), want)
    finally:
        r.close()


@forms()
def test_option_range(form):
    c = abi.Core(form.top, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="ARG"):
                c.set_option(form.option, bad)
        c.set_option(form.option, 1)
        c.set_option(form.option, 0)
    finally:
        c.finalize()


@cases("case", lambda f: f.ignored, ids=lambda case: case[0])
def test_ignored_sizes(form, case):
    """The ensemble sizes of the other paths (Form.ignored): accepted and ignored."""
    _, k, more, plain = case
    w = small(k)
    inp = Inputs(w)
    want, = off(inp, [w.var], opts=more)
    r = run(form, inp, more)
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            miss(info)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert plain in kt, kt
        assert not form.cached(kt), kt
    finally:
        r.close()


@forms(*HANDOFF)
def test_ignored_without_the_hand_off(form):
    """big_path = 0 at the form's largest k (one 256-thread kernel): accepted and ignored."""
    w = small(form.top)
    inp = Inputs(w)
    want, = off(inp, [w.var], opts={"big_path": 0})
    r = run(form, inp, {"big_path": 0})
    try:
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            miss(info)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
    finally:
        r.close()


@forms(ROWS)
def test_big_reuse_alone_keeps_nothing(form):
    """big_reuse = 1 without rows_reuse at k = 128: the path's own kernels, nothing held."""
    w = small(128)
    r = Run(Inputs(w), opts={"max_batch": 256, "big_reuse": 1}, base={})
    n = form.names(128)
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            miss(info)
            assert info["bytes_held"] == 0, info
            same((out, cnt), small_refs(128)[0])
        kt = r.c.kernel_times()
        assert n.head in kt and n.plain in kt and n.fill not in kt and n.hit not in kt, kt
    finally:
        r.close()


# ---- parity -----------------------------------------------------------------------------------
@forms()
def test_hit_against_the_oracle(form):
    """Both paths wrong alike would pass everything above: a hit against the oracle at the
    project's 1e-6 bar."""
    w = small(form.top)
    r = run(form, Inputs(w))
    try:
        miss(r.call(w.var)[2])
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
    finally:
        r.close()
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    ref = w.var.copy()
    ost = abi.Stats()
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, w.alt, ref)), 16, C.byref(ost))
    assert rc == 0
    assert cnt["solved"] == ost.solved and cnt["nobs_sum"] == ost.nobs_sum
    rel = increment_rel_rms(out, ref, w.var)
    moved = np.count_nonzero(bits(ref) != bits(w.var))
    print(f"k={form.top} hit: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= 1e-6, rel
