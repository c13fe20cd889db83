"""GPU tests of factor reuse in the record cache (CWBL_OPT_FACTOR_REUSE, on by default).

The call that fills the cache solves with fill_tq40_factor_kernel, which leaves each point's
factor A = Q T Q^T in the 860 words its record had; a hit solves with solve_tq40_factor_kernel
from those and skips the tridiagonalisation.  Both evaluate, for the analysed variable, the
expressions solve_tq40_kernel evaluates on the same bits, so every comparison here is exact
(np.array_equal on the bit patterns, equal counters) against the analysis with record_reuse = 0,
which runs solve_tq40_kernel on freshly assembled records.  reuse_info and the kernel timing
names show that the calls took the path the test means.

Workloads: test_gpu_record_reuse.py's (synth c2 at scale 0.1, batches of 1024 points in record
sub-batches of 512) and smaller ones where the case allows.
"""
import copy

import numpy as np
import pytest

from cwbl import abi, synth

import spectra_cases as sc
from reuse_harness import (Inputs, Run, bits, is_hit, is_miss, no_reuse, other_var, same)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL, HIT, PLAIN = "fill_tq40_factor_kernel<40>", "solve_tq40_factor_kernel<40>", "solve_tq40_kernel<40, 0>"
SMALL = {"max_batch": 256, "split40_batch": 128}


@pytest.fixture(scope="module")
def w():
    return synth.make("c2", scale=0.1)


@pytest.fixture(scope="module")
def var2(w):
    return other_var(w, 7)


@pytest.fixture(scope="module")
def refs(w, var2):
    """The analyses of w.var and var2 without reuse; shared, never modified."""
    return no_reuse(Inputs(w), [w.var, var2])


def small():
    """12 x 12 x 5 points, k = 40, 120 obs: three batches of 256 points."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120)


def solves(kt):
    return sorted(n for n in kt if "tq40" in n)


def fill_then_hits(inp, variables, want, nhits=2, **kw):
    """A fill on variables[0], then nhits rounds of hits over all variables: every call equals
    `want` (the no-reuse analyses, in order).  Returns the fill's reuse_info."""
    r = Run(inp, **kw)
    try:
        out, cnt, info = r.call(variables[0])
        assert info["batches_reused"] == 0 and info["batches_assembled"] >= 1, info
        nbat = info["batches_assembled"]
        same((out, cnt), want[0])
        for _ in range(nhits):
            for var, ref in zip(variables, want):
                out, cnt, hinfo = r.call(var)
                is_hit(hinfo, nbat)
                same((out, cnt), ref)
        return info
    finally:
        r.close()


def test_fill_and_hits_run_the_factor_kernels(w, var2, refs):
    """Fill, a hit on the same variable, a hit on another one, and both again (a hit does not
    consume the factor): each equals no-reuse.  The fill ran the fill kernel on every point
    and each hit the factor kernel; solve_tq40_kernel ran in neither."""
    r = Run(Inputs(w))
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        same((out, cnt), refs[0])
        kt = r.c.kernel_times()
        assert solves(kt) == [FILL], kt
        assert kt[FILL]["points"] == w.points and kt[FILL]["launches"] == 88, kt
        r.c.set_kernel_timing(True)
        for var, ref in ((w.var, refs[0]), (var2, refs[1]), (w.var, refs[0]), (var2, refs[1])):
            out, cnt, info = r.call(var)
            is_hit(info, 44)
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert solves(kt) == [HIT], kt
        assert kt[HIT]["points"] == 4 * w.points and "assemble_record_kernel<40>" not in kt, kt
    finally:
        r.close()


def test_factor_reuse_off_keeps_records(w, var2, refs):
    """factor_reuse = 0: the cache keeps records and both the fill and the hit run
    solve_tq40_kernel, with the same bits as factor_reuse = 1 (the two tests share `refs`)."""
    r = Run(Inputs(w), opts={"factor_reuse": 0})
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        same((out, cnt), refs[0])
        out, cnt, info = r.call(var2)
        is_hit(info, 44)
        same((out, cnt), refs[1])
        assert solves(r.c.kernel_times()) == [PLAIN]
    finally:
        r.close()


def test_switching_the_option_voids_the_cache(w, refs):
    """A cache of records is not read as factors, nor the other way round: setting the option
    makes the next call a miss that refills in the new form."""
    r = Run(Inputs(w), opts={"factor_reuse": 0})
    try:
        is_miss(r.call(w.var)[2], 44)
        for value in (1, 0, 1):
            r.c.set_option("factor_reuse", value)
            out, cnt, info = r.call(w.var)
            is_miss(info, 44)
            same((out, cnt), refs[0])
            out, cnt, info = r.call(w.var)
            is_hit(info, 44)
            same((out, cnt), refs[0])
    finally:
        r.close()


@pytest.mark.parametrize("k", [17, 25, 33, 40])
def test_ensemble_sizes_of_the_record_path(k):
    """k = 40 and the padded sizes on KP = 40 (steps j >= k - 2 are exact no-ops; the rows past
    k of x are stored as zeros)."""
    wl = synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)
    inp = Inputs(wl)
    v2 = other_var(wl, 3)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    assert want[0][1]["solved"] > 0
    fill_then_hits(inp, [wl.var, v2], want, opts=SMALL)


@pytest.mark.parametrize("k", [16, 48])
def test_other_paths_run_as_before(k):
    """The one-wavefront path has no record cache: the option changes nothing there, no batch is
    ever reused and nothing is held."""
    wl = synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)
    inp = Inputs(wl)
    want, = no_reuse(inp, [wl.var], opts=SMALL)
    for value in (0, 1):
        o = dict(SMALL)
        o["factor_reuse"] = value
        r = Run(inp, opts=o)
        try:
            for _ in range(2):
                out, cnt, info = r.call(wl.var)
                assert info["batches_reused"] == 0 and info["bytes_held"] == 0, info
                same((out, cnt), want)
        finally:
            r.close()


@pytest.mark.parametrize("sub", [0, 50, 37])
def test_ragged_points_and_sub_batch_seams(sub):
    """13 x 11 columns (ix_lim) x 5 levels = 715 points, no multiple of four, in batches of 256:
    the last wave of a launch reads the spare slot.  Sub-batches of 50 and 37 points put a seam
    (the next sub-batch's first slot is this one's spare; written in place by the fill, after
    this sub-batch's launch) every 50 resp. 37 points, none at a multiple of four."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120)
    inp = Inputs(wl)
    inp.ix_lim = 13
    o = {"max_batch": 256, "split40_batch": sub}
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2], opts=o)
    assert want[0][1]["points"] == 715
    fill_then_hits(inp, [wl.var, v2], want, opts=o)


def test_empty_lists_stay_untouched():
    """Every 25th obs only: points with p = 0 and with p < k.  The points no obs reaches keep
    their input bits through the fill and the hits.  (test_gpu_record_reuse.py's sparse case:
    the 30 x 30 x 50 grid, which nine obs do not cover.)"""
    wl = synth.make("c2", scale=0.1)
    keep = np.arange(wl.obs.shape[0]) % 25 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    inp = Inputs(wl)
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2])
    assert 0 < want[0][1]["solved"] < wl.points
    assert want[0][1]["nobs_sum"] / want[0][1]["solved"] < wl.k
    untouched = np.all(bits(want[0][0]) == bits(wl.var), axis=0)
    assert untouched.sum() >= wl.points - want[0][1]["solved"]
    fill_then_hits(inp, [wl.var, v2], want)


def test_truncated_lists():
    """max_lz_pts = 6: every reached point's list truncates (Q4); the counters of a hit come
    from the cache and equal the fill's."""
    wl = small()
    inp = Inputs(wl)
    inp.tp.max_lz_pts = 6
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    assert want[0][1]["lz_truncated"] > 0
    fill_then_hits(inp, [wl.var, v2], want, opts=SMALL)


@pytest.mark.parametrize("c", [c for c in sc.RECORD if c.mixed], ids=sc.case_id)
def test_mixed_quadrature_classes(c):
    """Waves whose four points need different round counts (R = 4 and 8; 3 and 4): the wave's
    R comes from the levels of the four traces, which the factor's diagonal reproduces."""
    wl = sc.workload(c)
    ev = sc.evaluate(c)
    assert sc.mixed_fours(c, ev.levels) > 0
    inp = Inputs(wl)
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    assert want[0][1]["max_sweeps"] == ev.levels.max()
    fill_then_hits(inp, [wl.var, v2], want, opts=SMALL)


def test_spectrum_beyond_the_last_table():
    """M/m > 1e24 at the one analysed point (the other three have p = 0): level -24 from the
    fill and from the hit, counted in nonconverged both times."""
    from test_gpu_analyze_vars_spectra import block_workload
    wl, _, _ = block_workload(32, 46, 32)
    inp = Inputs(wl)
    want = no_reuse(inp, wl.vars)
    assert want[0][1]["nonconverged"] == 1 and want[0][1]["max_sweeps"] == 24
    fill_then_hits(inp, wl.vars, want)


def test_epilogue_changed_between_fill_and_hit(w, refs):
    """RTPP / RTPS flags and alphas act after the factor: changed between the fill and the hit
    they keep the hit, which equals no-reuse under the new settings."""
    inp, new = Inputs(w), Inputs(w)
    new.vp.use_rtpp, new.vp.rtpp_alpha = 0, 0.5
    new.vp.use_rtps, new.vp.rtps_alpha = 1, 0.7
    ref_new, = no_reuse(new, [w.var])
    assert not np.array_equal(bits(refs[0][0]), bits(ref_new[0]))
    r = Run(inp)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        same((out, cnt), refs[0])
        r.sync(new)
        out, cnt, info = r.call(w.var)
        is_hit(info, 44)
        same((out, cnt), ref_new)
        r.sync(inp)
        out, cnt, info = r.call(w.var)
        is_hit(info, 44)
        same((out, cnt), refs[0])
    finally:
        r.close()


def test_nan_and_inf_var_do_not_spoil_the_factor():
    """A variable with a NaN column and an Inf column: as the fill's variable and as a hit's.
    The result equals no-reuse bit for bit (NaN payloads included), and a clean variable
    afterwards is served from the same cache."""
    wl = small()
    inp = Inputs(wl)
    bad = wl.var.copy()
    bad[3, 2, 5, 7] = np.nan
    bad[11, 4, 1, 2] = np.inf
    want_bad, want_clean = no_reuse(inp, [bad, wl.var], opts=SMALL)
    finite_pts = np.all(np.isfinite(want_bad[0]), axis=0)
    assert 0 < finite_pts.sum() < wl.points
    fill_then_hits(inp, [bad, wl.var], [want_bad, want_clean], opts=SMALL)
    fill_then_hits(inp, [wl.var, bad], [want_clean, want_bad], opts=SMALL)


def test_partial_budget(w, var2, refs):
    """14 MiB: two batches are kept as factors, the other 42 are assembled and solved by
    solve_tq40_kernel in every call."""
    r = Run(Inputs(w), reuse=14)
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        same((out, cnt), refs[0])
        kt = r.c.kernel_times()
        assert solves(kt) == sorted([FILL, PLAIN]) and kt[FILL]["points"] == 2048, kt
        r.c.set_kernel_timing(True)
        for var, ref in ((w.var, refs[0]), (var2, refs[1]), (w.var, refs[0])):
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 2 and info["batches_assembled"] == 42, info
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert solves(kt) == sorted([PLAIN, HIT]) and kt[HIT]["points"] == 3 * 2048, kt
    finally:
        r.close()


@pytest.mark.parametrize("window", [256, 2500])
def test_info_window_rollover(w, var2, refs, window):
    fill_then_hits(Inputs(w), [w.var, var2], refs, nhits=1, opts={"info_window": window})


def test_host_slab(w, var2, refs):
    fill_then_hits(Inputs(w), [w.var, var2], refs, nhits=1, host=True)


def test_invalidation_then_refill_over_old_factors(w, refs):
    """After a fill and a hit an input of the record changes (hclr): the next call assembles
    new records into the buffer that holds the old factors, refills, and the call after it
    hits; then back again."""
    inp, new = Inputs(w), Inputs(w)
    new.tp.hclr = 10.0
    ref_new, = no_reuse(new, [w.var])
    assert not np.array_equal(bits(refs[0][0]), bits(ref_new[0]))
    r = Run(inp)
    try:
        is_miss(r.call(w.var)[2], 44)
        for cur, ref in ((new, ref_new), (inp, refs[0])):
            out, cnt, info = r.call(w.var)
            is_hit(info, 44)
            r.sync(cur)
            out, cnt, info = r.call(w.var)
            is_miss(info)
            same((out, cnt), ref)
            out, cnt, info = r.call(w.var)
            is_hit(info, info["batches_reused"])
            same((out, cnt), ref)
    finally:
        r.close()


def test_option_range():
    c = abi.Core(40, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="ARG"):
                c.set_option("factor_reuse", bad)
        c.set_option("factor_reuse", 0)
        c.set_option("factor_reuse", 1)
    finally:
        c.finalize()
