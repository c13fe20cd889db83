"""GPU tests of the factor cache of the one-wavefront path (CWBL_OPT_WAVE_REUSE, k = 41..64).

With the option on, a cwbl_analyze_var call whose key misses runs fill_tq_wave_kernel<KP>
(solve_tq_kernel<KP>'s analysis, which also leaves each point's factor A = Q T Q^T), and a
call with an equal key and bit-equal coordinates runs solve_tq_wave_factor_kernel<KP> on the
kept factors and nothing before it.  The fill is the single kernel's text and the hit replays
its x' expressions in its order, so every comparison of analyses here is exact
(np.array_equal on the bit patterns) and every comparison of counters is equality, against
the same inputs with the option off (record_reuse = 0 as well: test_gpu_record_reuse.no_reuse).

Workloads: 12 x 12 x 5 points with 120 obs in batches of 256, 256 and 208; 13 x 11 x 5 = 715
points (ix_lim < nx) for ragged ends.  Ensemble sizes 64, 56, 48 (k = KP) and 50 (KP = 56 with
six padding rows).  On this path the quadrature has two rules, 31 nodes (levels up to 12) and
63 nodes above: spectra_cases.WAVE's k = 64 cases hold both, each alone and mixed, and
block_workload(64, 46) the spectrum beyond the last table.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import spectra_cases as sc
from cwbl import abi, synth
from helpers import increment_rel_rms, oracle
from test_gpu_record_reuse import Inputs, Run, bits, no_reuse, other_var, same, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = [64, 56, 48, 50]
BATCH = {"max_batch": 256}
ON = {"max_batch": 256, "wave_reuse": 1}
SEARCH = ("search_binned_kernel", "search_flagged_kernel", "search_tree_kernel")


def kp_of(k):
    return (k + 7) // 8 * 8


def names(k):
    kp = kp_of(k)
    return (f"fill_tq_wave_kernel<{kp}>", f"solve_tq_wave_factor_kernel<{kp}>",
            f"solve_tq_kernel<{kp}, false>")


class WRun(Run):
    """test_gpu_record_reuse.Run with cwbl_init's further arguments (weight_function)."""

    def __init__(self, inp, reuse=None, opts=None, host=False, **core):
        options = dict(opts or {})
        if reuse is not None:
            options["record_reuse"] = reuse
        self.c = abi.Core(inp.k, device=0, options=options, **core)
        self.host = host
        self.inp = inp
        self.x, self.y, self.alt = (a.copy() if host else to_dev(a) for a in (inp.x, inp.y, inp.alt))
        self.hdxb = None
        self.applied = {}
        self.sync(inp)


def off(inp, variables, opts=None, **core):
    """The analyses of `variables` with wave_reuse = 0 and record_reuse = 0: [(out, counters)]."""
    if not core:
        return no_reuse(inp, variables, opts=dict(BATCH, **(opts or {})))
    r = WRun(inp, reuse=0, opts=dict(BATCH, **(opts or {})), **core)
    try:
        outs = []
        for var in variables:
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 0 and info["bytes_held"] == 0, info
            outs.append((out, cnt))
        return outs
    finally:
        r.close()


def is_miss(info, nbat):
    assert info["batches_reused"] == 0 and info["batches_assembled"] == nbat, info


def is_hit(info, nbat):
    assert info["batches_reused"] == nbat and info["batches_assembled"] == 0, info
    assert info["bytes_held"] > 0, info


def fill_then_hits(inp, variables, want, nbat=3, opts=None, host=False, points=None, **core):
    """A fill on variables[0], then a hit on every variable: each call equals `want` (the
    analyses with the option off, in order), counters included; the hits ran the hit kernel
    over all `points`, once per batch, and neither a search nor solve_tq_kernel."""
    r = WRun(inp, opts=dict(ON, **(opts or {})), host=host, **core)
    fill, hit, plain = names(inp.k)
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(variables[0])
        is_miss(info, nbat)
        same((out, cnt), want[0])
        kt = r.c.kernel_times()
        assert fill in kt and hit not in kt and plain not in kt, kt
        assert kt[fill]["launches"] == nbat, kt
        r.c.set_kernel_timing(True)
        for var, ref in zip(variables, want):
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert sorted(n for n in kt if n != "tune_q_kernel") == [hit], kt
        assert kt[hit]["launches"] == nbat * len(variables), kt
        if points is not None:
            assert kt[hit]["points"] == points * len(variables), kt
        return info
    finally:
        r.close()


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


# ---- fill and hit -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_fill_and_hits(k):
    """Fill with one variable, hit with it and with two others; the factor's bytes are held."""
    w = small(k)
    want = small_refs(k)
    assert want[0][1]["solved"] > 0 and want[0][1]["points"] == 720
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    info = fill_then_hits(Inputs(w), [w.var, other_var(w, 5), other_var(w, 6)], want, points=720)
    kp = kp_of(k)
    words = kp * (kp - 1) // 2 + 5 * kp
    # every batch's factors and its spare one, the accepted counts, the snapshot
    assert info["bytes_held"] >= (720 + 3) * words * 8 + 8 * 720, info


@pytest.mark.parametrize("k", KS)
def test_per_call_epilogue(k):
    """The hit call's RTPP / RTPS flags and alphas and tune_q, not the fill's."""
    w = small(k)
    inp, new = Inputs(w), Inputs(w)
    new.vp.use_rtpp, new.vp.rtpp_alpha = 0, 0.5
    new.vp.use_rtps, new.vp.rtps_alpha = 1, 0.7
    new.vp.tune_q = 1
    ref_new, = off(new, [w.var])
    assert not np.array_equal(bits(small_refs(k)[0][0]), bits(ref_new[0]))
    r = WRun(inp, opts=ON)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
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
@pytest.mark.parametrize("k", KS)
def test_sparse_obs_and_untouched_points(k):
    """Every 40th obs: points with p = 0, which keep their input bits through the fill and the
    hits, and points with p < k (exactly-zero reflectors: the tau = 0 branch)."""
    wl = sparse(k)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    cnt = want[0][1]
    assert 0 < cnt["solved"] < wl.points and cnt["nobs_sum"] / cnt["solved"] < k
    for (out, _), var in zip(want, variables):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() == wl.points - cnt["solved"]
    fill_then_hits(inp, variables, want)


@pytest.mark.parametrize("k", [64, 50])
def test_truncated_lists(k):
    """max_lz_pts = 6: every reached list truncates; a hit's counters come from the cache."""
    wl = small(k)
    inp = Inputs(wl)
    inp.tp.max_lz_pts = 6
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    assert want[0][1]["lz_truncated"] > 0
    fill_then_hits(inp, variables, want)


@pytest.mark.parametrize("k", [64, 50])
def test_gaspari_cohn_nans(k):
    """weight_function = 1: the reference's fp32 Gaspari-Cohn weights give NaN factors at some
    points; the hit reproduces the fill's NaNs bit for bit."""
    wl = small(k)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables, weight_function=1)
    assert not np.array_equal(bits(want[0][0]), bits(small_refs(k)[0][0]))
    print(f"gaspari-cohn k={k}: {int(np.isnan(want[0][0]).any(axis=0).sum())} NaN points")
    fill_then_hits(inp, variables, want, weight_function=1)


@pytest.mark.parametrize("k", [64, 50])
def test_nan_and_inf_members(k):
    """A variable with a NaN member and an Inf member, as the fill's variable and as a hit's."""
    wl = small(k)
    inp = Inputs(wl)
    bad = wl.var.copy()
    bad[3, 2, 5, 7] = np.nan
    bad[11, 4, 1, 2] = np.inf
    want_bad, = off(inp, [bad])
    want_clean = small_refs(k)[0]
    finite = np.all(np.isfinite(want_bad[0]), axis=0)
    assert 0 < finite.sum() < wl.points
    fill_then_hits(inp, [bad, wl.var], [want_bad, want_clean])
    fill_then_hits(inp, [wl.var, bad], [want_clean, want_bad])


# ---- quadrature rules -------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in sc.WAVE if c.k == 64], ids=sc.case_id)
def test_wide_spectra(c):
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
    fill_then_hits(inp, variables, want)


def test_spectrum_beyond_the_last_table():
    """M/m > 1e24 at the one analysed point (three more with p = 0): level -24 from the fill
    and from the hit, counted in nonconverged both times."""
    from test_gpu_analyze_vars_spectra import block_workload
    wl, _, _ = block_workload(64, 46, 64)
    inp = Inputs(wl)
    want = off(inp, wl.vars)
    assert want[0][1]["nonconverged"] == 1 and want[0][1]["max_sweeps"] == 24
    fill_then_hits(inp, wl.vars, want, nbat=1)


# ---- slab kinds -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged(k):
    return synth.make("c2", seed=11, nx=14, ny=11, nz=5, n_obs=120, k=k)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("k", [64, 50])
def test_ragged_points(k, host):
    """13 (ix_lim) x 11 x 5 = 715 points of a 14-column slab, batches of 256, 256 and 203; from
    device memory and from a pageable host slab."""
    wl = ragged(k)
    inp = Inputs(wl)
    inp.ix_lim = 13
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    assert want[0][1]["points"] == 715 and want[0][1]["solved"] > 0
    fill_then_hits(inp, variables, want, host=host, points=715)


@pytest.mark.parametrize("k", [64, 48])
def test_host_slab(k):
    """A pageable host slab whose analysed region is the whole slab (var is piped batch by
    batch): fill, hits, and a miss after the caller rewrote alt in place."""
    w = small(k)
    want = small_refs(k)
    r = WRun(Inputs(w), opts=ON, host=True)
    try:
        fill = r.call(w.var)
        is_miss(fill[2], 3)
        same(fill[:2], want[0])
        for var, ref in ((w.var, want[0]), (other_var(w, 5), want[1])):
            hit = r.call(var)
            is_hit(hit[2], 3)
            same(hit[:2], ref)
        r.alt += np.float32(37.0)
        is_miss(r.call(w.var)[2], 3)
    finally:
        r.close()


@pytest.mark.parametrize("window", [256, 600])
def test_small_info_window(window):
    """One info window per batch (256) and a rollover inside the call (600): the hit restores
    the accepted counts window by window."""
    w = small(64)
    fill_then_hits(Inputs(w), [w.var, other_var(w, 5)], small_refs(64)[:2],
                   opts={"info_window": window})


def test_device_built_index():
    """index = 1: a full hit needs neither the bins nor a tree."""
    w = small(64)
    inp = Inputs(w)
    variables = [w.var, other_var(w, 5)]
    want = off(inp, variables, opts={"index": 1})
    fill_then_hits(inp, variables, want, opts={"index": 1})


# ---- misses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 48])
def test_partial_budget(k):
    """A budget that holds the first of three batches (257 factors) and not the second: later
    calls reuse that one, search and solve the other two with solve_tq_kernel."""
    w = small(k)
    kp = kp_of(k)
    per = (kp * (kp - 1) // 2 + 5 * kp) * 8
    mib = (257 * per >> 20) + 1
    assert 257 * per <= mib << 20 < 2 * 257 * per
    want = small_refs(k)
    r = WRun(Inputs(w), reuse=mib, opts=ON)
    fill, hit, plain = names(k)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        assert 257 * per <= info["bytes_held"] < 2 * 257 * per
        same((out, cnt), want[0])
        r.c.set_kernel_timing(True)
        for var, ref in ((w.var, want[0]), (other_var(w, 5), want[1])):
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 1 and info["batches_assembled"] == 2, info
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert kt[hit]["points"] == 2 * 256 and kt[plain]["points"] == 2 * (720 - 256), kt
        assert fill not in kt, kt
    finally:
        r.close()


def test_budget_of_zero_turns_the_cache_off():
    w = small(64)
    r = WRun(Inputs(w), reuse=0, opts=ON)
    try:
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), small_refs(64)[0])
    finally:
        r.close()


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


@pytest.mark.parametrize("what", sorted(CHANGES))
def test_invalidation(what):
    """After a fill and a hit one input of the factor changes: a miss that equals the analysis
    of the new inputs with the option off, refilled over the old factors, then a hit again."""
    w = small(64)
    inp, new = Inputs(w), Inputs(w)
    CHANGES[what](new, w)
    ref_old = small_refs(64)[0]
    ref_new, = off(new, [w.var])
    assert not np.array_equal(bits(ref_old[0]), bits(ref_new[0]))
    r = WRun(inp, opts=ON)
    try:
        is_miss(r.call(w.var)[2], 3)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), ref_old)
        r.sync(new)
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        same((out, cnt), ref_new)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), ref_new)
    finally:
        r.close()


# ---- calls that bypass the cache --------------------------------------------------------------
def test_group_call_leaves_the_cache_valid():
    w = small(64)
    want = small_refs(64)
    r = WRun(Inputs(w), opts=ON)
    try:
        is_miss(r.call(w.var)[2], 3)
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


def test_column_share_call_leaves_the_cache_valid():
    """test_gpu_column_share.test_cache_untouched at k = 64: a per-point call (a 3-D type)
    fills, a column-shared call with other type parameters follows, the first call hits."""
    from test_gpu_analyze_vars import Lib
    from test_gpu_column_share import workload
    w3, w2 = workload(64, 9, "3d"), workload(64, 9, "dense")
    ref3, = no_reuse(Inputs(w3), [w3.var], opts=BATCH)
    lib = Lib(w3, dict(ON, column_share=1), reuse_default=True)
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
def test_toggling_the_option_invalidates_and_releases():
    w = small(64)
    want = small_refs(64)[0]
    r = WRun(Inputs(w), opts=ON)
    _, hit, plain = names(64)
    try:
        is_miss(r.call(w.var)[2], 3)
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option("wave_reuse", 0)
        r.c.set_kernel_timing(True)
        for _ in range(2):  # option 0: nothing reused, nothing held, the path's own kernels
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert plain in kt and not [n for n in kt if "wave" in n], kt
        r.c.set_option("wave_reuse", 1)
        is_miss(r.call(w.var)[2], 3)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), want)
    finally:
        r.close()


def test_option_range():
    c = abi.Core(64, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="ARG"):
                c.set_option("wave_reuse", bad)
        c.set_option("wave_reuse", 1)
        c.set_option("wave_reuse", 0)
    finally:
        c.finalize()


@pytest.mark.parametrize("k,more", [(16, {}), (40, {"split40": 0})])
def test_ignored_sizes(k, more):
    """k <= 16, and k = 17..40 without the record split: accepted and ignored."""
    w = small(k)
    inp = Inputs(w)
    want, = off(inp, [w.var], opts=more)
    r = WRun(inp, opts=dict(ON, **more))
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert f"solve_tq_kernel<{kp_of(k)}, false>" in kt, kt
        assert not [n for n in kt if "wave" in n], kt
    finally:
        r.close()


# ---- parity -----------------------------------------------------------------------------------
def test_hit_against_the_oracle():
    """Both paths wrong alike would pass everything above: a hit against the oracle at the
    project's 1e-6 bar."""
    w = small(64)
    r = WRun(Inputs(w), opts=ON)
    try:
        is_miss(r.call(w.var)[2], 3)
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
    print(f"k=64 hit: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= 1e-6, rel
