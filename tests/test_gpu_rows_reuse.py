"""GPU tests of the factor cache of the hand-off path at k = 97..128 (CWBL_OPT_ROWS_REUSE).

With the option on, a cwbl_analyze_var call whose key misses runs the half-row hand-off kernel
solve_tq_rows_kernel<128, 64> unchanged and fill_tqb_tail_kernel<128, 64> in the tail's place
(solve_tqb_tail_kernel<128, 64, 3>'s analysis, which also leaves each point's factor
A = Q T Q^T), and a call with an equal key and bit-equal coordinates runs
solve_tqb_factor_kernel<128, 64> on the kept factors and nothing before it.  The fill is the
tail's text and the hit replays the x' expressions of both kernels in their order, so every
comparison of analyses here is exact (np.array_equal on the bit patterns) and every comparison
of counters is equality, against the same inputs with the option off (record_reuse = 0 as
well: test_gpu_record_reuse.no_reuse).

Workloads: 12 x 12 x 5 points with 120 obs in batches of 256, 256 and 208; 13 x 11 x 5 = 715
points (ix_lim < nx) for ragged ends.  Ensemble sizes 128 (no padding rows), 112 and 97 (31
padding rows and the shortest tail: 31 steps).  The quadrature has two rules, 31 nodes (levels
up to 12) and 63 nodes above: spectra_cases.BIG's k = 128 cases hold both, each alone and mixed.
"""
import ctypes as C

import numpy as np
import pytest

import spectra_cases as sc
from cwbl import abi
from helpers import increment_rel_rms, oracle
from test_gpu_record_reuse import Inputs, bits, no_reuse, other_var, same, to_dev
from test_gpu_wave_reuse import (BATCH, CHANGES, WRun, is_hit, is_miss, off, ragged, small,
                                 small_refs, sparse)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = [128, 112, 97]
ON = {"max_batch": 256, "rows_reuse": 1}
HEAD = "solve_tq_rows_kernel<128, 64>"
TAIL = "solve_tqb_tail_kernel<128, 64, 3>"
FILL = "fill_tqb_tail_kernel<128, 64>"
HIT = "solve_tqb_factor_kernel<128, 64>"
WORDS = 128 * 127 // 2 + 5 * 128  # the bound on a factor's fp64 words; BigFactor<128, 64> has 8705
FACTOR_WORDS = 8705


def fill_then_hits(inp, variables, want, nbat=3, nsub=1, opts=None, host=False, points=None,
                   **core):
    """A fill on variables[0], then a hit on every variable: each call equals `want` (the
    analyses with the option off, in order), counters included; the fill ran the hand-off
    kernel and the fill tail, the hits ran the hit kernel over all `points`, once per cached
    sub-batch (nsub per batch), and neither a search, the hand-off kernel nor the tail."""
    r = WRun(inp, opts=dict(ON, **(opts or {})), host=host, **core)
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(variables[0])
        is_miss(info, nbat)
        same((out, cnt), want[0])
        kt = r.c.kernel_times()
        assert HEAD in kt and FILL in kt and HIT not in kt and TAIL not in kt, kt
        assert kt[FILL]["launches"] == nbat * nsub == kt[HEAD]["launches"], kt
        r.c.set_kernel_timing(True)
        for var, ref in zip(variables, want):
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            same((out, cnt), ref)
        kt = r.c.kernel_times()
        assert sorted(n for n in kt if n != "tune_q_kernel") == [HIT], kt
        assert kt[HIT]["launches"] == nbat * nsub * len(variables), kt
        if points is not None:
            assert kt[HIT]["points"] == points * len(variables), kt
        return info
    finally:
        r.close()


# ---- fill and hit -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_fill_and_hits(k):
    """Fill with one variable, hit with it and with two others; the factor's bytes are held."""
    w = small(k)
    want = small_refs(k)
    assert want[0][1]["solved"] > 0 and want[0][1]["points"] == 720
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    info = fill_then_hits(Inputs(w), [w.var, other_var(w, 5), other_var(w, 6)], want, points=720)
    # every batch's factors and its spare one, the accepted counts, the snapshot
    assert info["bytes_held"] >= (720 + 3) * FACTOR_WORDS * 8 + 8 * 720, info
    assert info["bytes_held"] < (720 + 3) * WORDS * 8 * (1 + 1 / 16) + (1 << 16), info


@pytest.mark.parametrize("k", KS)
def test_sub_batches(k):
    """big_batch = 128: every cached batch keeps two sub-batches' factors (128 + 128, 128 + 80),
    and a hit is one launch per sub-batch."""
    w = small(k)
    variables = [w.var, other_var(w, 5)]
    want = off(Inputs(w), variables, opts={"big_batch": 128})
    same(want[0], small_refs(k)[0])
    fill_then_hits(Inputs(w), variables, want, nsub=2, opts={"big_batch": 128}, points=720)


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
    """Every 40th obs (three are left): points with p = 0, which keep their input bits through
    the fill and the hits, and points with p = 1 and p = 2, whose steps past the first ones are
    exactly-zero reflectors (tau = 0) in the hand-off kernel's half and in the tail's."""
    wl = sparse(k)
    inp = Inputs(wl)
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    cnt = want[0][1]
    print(f"sparse k={k}: {cnt['solved']} points solved, {cnt['nobs_sum']} obs accepted, "
          f"max_p {cnt['max_p']}")
    # p <= 3 everywhere (three obs), some point with p >= 2 and some point with p < max_p
    assert 0 < cnt["solved"] < wl.points and 2 <= cnt["max_p"] <= 3
    assert cnt["solved"] < cnt["nobs_sum"] < cnt["max_p"] * cnt["solved"]
    for (out, _), var in zip(want, variables):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() == wl.points - cnt["solved"]
    fill_then_hits(inp, variables, want)


@pytest.mark.parametrize("k", [128, 97])
def test_truncated_lists(k):
    """max_lz_pts = 6: every reached list truncates; a hit's counters come from the cache."""
    wl = small(k)
    inp = Inputs(wl)
    inp.tp.max_lz_pts = 6
    variables = [wl.var, other_var(wl, 5)]
    want = off(inp, variables)
    assert want[0][1]["lz_truncated"] > 0
    fill_then_hits(inp, variables, want)


@pytest.mark.parametrize("k", [128, 97])
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


@pytest.mark.parametrize("k", [128, 97])
def test_nan_and_inf_members(k):
    """A variable with a NaN member and an Inf member, one in rows < 64 and one in rows >= 64
    (the two halves of the hand-off kernel's v . x' sum), as the fill's variable and as a hit's;
    and the two swapped."""
    wl = small(k)
    inp = Inputs(wl)
    bad = wl.var.copy()
    bad[3, 2, 5, 7] = np.nan
    bad[70, 4, 1, 2] = np.inf
    swap = wl.var.copy()
    swap[3, 2, 5, 7] = np.inf
    swap[70, 4, 1, 2] = np.nan
    want_bad, want_swap = off(inp, [bad, swap])
    want_clean = small_refs(k)[0]
    for want in (want_bad, want_swap):
        finite = np.all(np.isfinite(want[0]), axis=0)
        assert 0 < finite.sum() < wl.points
    fill_then_hits(inp, [bad, wl.var, swap], [want_bad, want_clean, want_swap])
    fill_then_hits(inp, [wl.var, bad], [want_clean, want_bad])


# ---- quadrature rules -------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in sc.BIG if c.k == 128], ids=sc.case_id)
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


# ---- slab kinds -------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("k", [128, 97])
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


@pytest.mark.parametrize("k", [128, 112])
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
    w = small(128)
    fill_then_hits(Inputs(w), [w.var, other_var(w, 5)], small_refs(128)[:2],
                   opts={"info_window": window})


def test_device_built_index():
    """index = 1: a full hit needs neither the bins nor a tree."""
    w = small(128)
    inp = Inputs(w)
    variables = [w.var, other_var(w, 5)]
    want = off(inp, variables, opts={"index": 1})
    fill_then_hits(inp, variables, want, opts={"index": 1})


# ---- misses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [128, 97])
def test_partial_budget(k):
    """A budget that holds the first of three batches (257 factors) and not the second: later
    calls reuse that one, search and solve the other two with the kernel pair."""
    w = small(k)
    per = FACTOR_WORDS * 8
    mib = (257 * per >> 20) + 1
    assert 257 * per <= mib << 20 < 2 * 257 * per
    want = small_refs(k)
    r = WRun(Inputs(w), reuse=mib, opts=ON)
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
        assert kt[HIT]["points"] == 2 * 256 and kt[TAIL]["points"] == 2 * (720 - 256), kt
        assert kt[HEAD]["points"] == 2 * (720 - 256) and FILL not in kt, kt
    finally:
        r.close()


def test_budget_of_zero_turns_the_cache_off():
    w = small(128)
    r = WRun(Inputs(w), reuse=0, opts=ON)
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), small_refs(128)[0])
        kt = r.c.kernel_times()
        assert TAIL in kt and FILL not in kt and HIT not in kt, kt
    finally:
        r.close()


@pytest.mark.parametrize("what", sorted(CHANGES))
def test_invalidation(what):
    """After a fill and a hit one input of the factor changes (the obs set, a coordinate
    rewritten in place, a type parameter, multi_infl): a miss that equals the analysis of the new
    inputs with the option off, refilled over the old factors, then a hit again."""
    w = small(128)
    inp, new = Inputs(w), Inputs(w)
    CHANGES[what](new, w)
    ref_old = small_refs(128)[0]
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


def test_option_change_invalidates():
    """Any generation-bumping option voids the factors: big_batch changes the sub-batches."""
    w = small(128)
    want = small_refs(128)[0]
    r = WRun(Inputs(w), opts=ON)
    try:
        is_miss(r.call(w.var)[2], 3)
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option("big_batch", 128)
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        same((out, cnt), want)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), want)
    finally:
        r.close()


# ---- calls that bypass the cache --------------------------------------------------------------
def test_group_call_leaves_the_cache_valid():
    w = small(128)
    want = small_refs(128)
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
    """test_gpu_column_share.test_cache_untouched at k = 128: a per-point call (a 3-D type)
    fills, a column-shared call with other type parameters follows, the first call hits."""
    from test_gpu_analyze_vars import Lib
    from test_gpu_column_share import workload
    w3, w2 = workload(128, 9, "3d"), workload(128, 9, "dense")
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
    w = small(128)
    want = small_refs(128)[0]
    r = WRun(Inputs(w), opts=ON)
    try:
        is_miss(r.call(w.var)[2], 3)
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option("rows_reuse", 0)
        r.c.set_kernel_timing(True)
        for _ in range(2):  # option 0: nothing reused, nothing held, the path's own kernels
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert HEAD in kt and TAIL in kt and FILL not in kt and HIT not in kt, kt
        r.c.set_option("rows_reuse", 1)
        is_miss(r.call(w.var)[2], 3)
        out, cnt, info = r.call(w.var)
        is_hit(info, 3)
        same((out, cnt), want)
    finally:
        r.close()


def test_option_range():
    c = abi.Core(128, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="ARG"):
                c.set_option("rows_reuse", bad)
        c.set_option("rows_reuse", 1)
        c.set_option("rows_reuse", 0)
    finally:
        c.finalize()


@pytest.mark.parametrize("k,plain", [(96, "solve_tqb_tail_kernel<96, 32, 2>"),
                                     (64, "solve_tq_kernel<64, false>")])
def test_ignored_sizes(k, plain):
    """k = 65..96 and k <= 64: accepted and ignored."""
    w = small(k)
    inp = Inputs(w)
    want, = off(inp, [w.var])
    r = WRun(inp, opts=ON)
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
        kt = r.c.kernel_times()
        assert plain in kt, kt
        assert not [n for n in kt if "fill" in n or "factor" in n], kt
    finally:
        r.close()


def test_ignored_without_the_hand_off():
    """big_path = 0 at k = 128 (one 256-thread kernel): accepted and ignored."""
    w = small(128)
    inp = Inputs(w)
    want, = off(inp, [w.var], opts={"big_path": 0})
    r = WRun(inp, opts=dict(ON, big_path=0))
    try:
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
    finally:
        r.close()


def test_big_reuse_alone_keeps_nothing():
    """big_reuse = 1 without rows_reuse at k = 128: the path's own kernels, nothing held."""
    w = small(128)
    r = WRun(Inputs(w), opts={"max_batch": 256, "big_reuse": 1})
    try:
        r.c.set_kernel_timing(True)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), small_refs(128)[0])
        kt = r.c.kernel_times()
        assert HEAD in kt and TAIL in kt and FILL not in kt and HIT not in kt, kt
    finally:
        r.close()


# ---- parity -----------------------------------------------------------------------------------
def test_hit_against_the_oracle():
    """Both paths wrong alike would pass everything above: a hit against the oracle at the
    project's 1e-6 bar."""
    w = small(128)
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
    print(f"k=128 hit: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= 1e-6, rel
