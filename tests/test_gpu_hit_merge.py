"""GPU tests of the merged hit launch (CWBL_OPT_HIT_MERGE, on by default).

A call that solves from the factor cache issues one launch of solve_tq40_factor_merged_kernel
per info window for all its cached batches, instead of one launch of solve_tq40_factor_kernel
per cached batch or sub-batch.  Row y of the merged grid is the segment that launch y of the
per-batch form covers, so every wave holds the same four points and runs the same text on the
same bits: every comparison here is exact (np.array_equal on the bit patterns, equal counters),
against hit_merge = 0 and against record_reuse = 0 (both forms are compared with the same
no-reuse analysis).  reuse_info and the kernel timing show the path each call took.

Workloads: test_gpu_factor_reuse.py's.
"""
import numpy as np
import pytest

from cwbl import abi, synth

from reuse_harness import Inputs, Run, bits, is_hit, is_miss, no_reuse, other_var, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HIT, MERGED = "solve_tq40_factor_kernel<40>", "solve_tq40_factor_merged_kernel<40>"
PLAIN, FILL = "solve_tq40_kernel<40, 0>", "fill_tq40_factor_kernel<40>"
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


def small(**kw):
    """12 x 12 x 5 points, k = 40, 120 obs: 720 points, batches of 256, 256 and 208."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, **kw)


def hit_launches(kt):
    """(launches, points) of the hit kernel in kernel times: the merged launches are reported
    under the hit kernel's name."""
    assert MERGED not in kt, kt
    t = kt.get(HIT, {"launches": 0, "points": 0})
    return t["launches"], t["points"]


def fill_then_hits(inp, variables, want, merge, opts=None, nhits=1, launches=None, cached=None,
                   reused=None, **kw):
    """A fill on variables[0], then nhits rounds of hits over all variables under hit_merge =
    `merge`: every call equals `want` (the no-reuse analyses, in order).  launches: hit-kernel
    launches per hit call, cached: the points each of them covers in all; reused: cached
    batches when the budget does not hold every one."""
    o = dict(opts or {})
    o["hit_merge"] = merge
    r = Run(inp, opts=o, **kw)
    try:
        out, cnt, info = r.call(variables[0])
        is_miss(info)
        nbat = info["batches_assembled"]
        same((out, cnt), want[0])
        r.c.set_kernel_timing(True)
        ncall = 0
        for _ in range(nhits):
            for var, ref in zip(variables, want):
                out, cnt, info = r.call(var)
                if reused is None:
                    is_hit(info, nbat)
                else:
                    assert info["batches_reused"] == reused, info
                    assert info["batches_assembled"] == nbat - reused, info
                same((out, cnt), ref)
                ncall += 1
        kt = r.c.kernel_times()
        n, pts = hit_launches(kt)
        print(f"hit_merge={merge}: {n} hit launches over {ncall} calls, {pts} points")
        if launches is not None:
            assert n == launches * ncall, kt
        if cached is not None:
            assert pts == cached * ncall, kt
        return nbat, kt
    finally:
        r.close()


def test_three_batches():
    """720 points in batches of 256, 256 and 208: three segments, the last one shorter than
    the grid's rows.  One fill, two hits with different var: a merged hit is one launch over
    the 720 cached points, hit_merge = 0 is three."""
    wl = small()
    inp = Inputs(wl)
    v2 = other_var(wl, 5)
    o = {"max_batch": 256}
    want = no_reuse(inp, [wl.var, v2], opts=o)
    assert want[0][1]["points"] == 720 and want[0][1]["solved"] > 0
    nbat, _ = fill_then_hits(inp, [wl.var, v2], want, 1, opts=o, launches=1, cached=720)
    assert nbat == 3
    fill_then_hits(inp, [wl.var, v2], want, 0, opts=o, launches=3, cached=720)


# 715 points in batches of 256, 256 and 203; (sub-batch size, segments of the three batches)
RAGGED = [(0, 3), (50, 4 + 4 + 4), (37, 4 + 4 + 4)]


@pytest.mark.parametrize("sub,nseg", RAGGED)
@pytest.mark.parametrize("host", [False, True])
def test_ragged_seams(sub, nseg, host):
    """13 x 11 columns (ix_lim) x 5 levels = 715 points, no multiple of four, in batches of 256
    and sub-batches of 50 or 37 points (sub_batch splits evenly and rounds up to a whole list
    group, so both give sub-batches of 64 points; the last one of the 203-point batch has 11,
    and 203 is no multiple of four either).  The last wave of every ragged segment reads
    the segment's spare record and aux entry, and no wave mixes points of two segments: a wave
    that did would run the largest rule of other four points and change bits.  host: a host
    slab with ix_lim < nx is staged whole, so the call merges as well."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120)
    inp = Inputs(wl)
    inp.ix_lim = 13
    o = {"max_batch": 256, "split40_batch": sub}
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2], opts=o)
    assert want[0][1]["points"] == 715
    fill_then_hits(inp, [wl.var, v2], want, 1, opts=o, launches=1, cached=715, host=host)
    fill_then_hits(inp, [wl.var, v2], want, 0, opts=o, launches=nseg, cached=715, host=host)


def test_batch_size_no_multiple_of_four():
    """max_batch = 270 (the option takes no value below 256): plan_batches rounds a batch up to
    whole list groups of 64 points (720 points in three batches: 240 -> 256, 256, 208), so a
    batch size that is no multiple of four does not occur; the ragged segments are the last
    batch's and the sub-batches' (see test_ragged_seams).  The rounded plan under the merged
    launch: same bits."""
    wl = small()
    inp = Inputs(wl)
    o = {"max_batch": 270}
    want = no_reuse(inp, [wl.var], opts=o)
    nbat, _ = fill_then_hits(inp, [wl.var], want, 1, opts=o, launches=1, cached=720)
    assert nbat == 3


@pytest.mark.parametrize("sub", [512, 100])
def test_info_windows(sub):
    """info_window = 512 on 720 points: the windows are [0, 512) and [512, 720), one merged
    launch each (two batches, then one), with whole batches and with sub-batches."""
    wl = small()
    inp = Inputs(wl)
    v2 = other_var(wl, 5)
    o = {"max_batch": 256, "split40_batch": sub, "info_window": 512}
    want = no_reuse(inp, [wl.var, v2], opts=o)
    fill_then_hits(inp, [wl.var, v2], want, 1, opts=o, launches=2, cached=720)
    per_batch = 3 if sub == 512 else 2 + 2 + 2
    fill_then_hits(inp, [wl.var, v2], want, 0, opts=o, launches=per_batch, cached=720)


def test_partial_budget(w, var2, refs):
    """14 MiB hold two of the 44 batches: the two are one merged launch (2048 points), the
    third batch's search is queued ahead of it, and the other 42 are assembled and solved per
    batch by solve_tq40_kernel, in every call."""
    for merge, launches in ((1, 1), (0, 4)):
        _, kt = fill_then_hits(Inputs(w), [w.var, var2], refs, merge, reuse=14, reused=2,
                               launches=launches, cached=2048)
        assert kt[PLAIN]["points"] == 2 * (w.points - 2048), kt


@pytest.mark.parametrize("k", [17, 33])
def test_k_below_40(k):
    """k = 17 and 33 on KP = 40 (rows past k masked)."""
    wl = small(k=k)
    inp = Inputs(wl)
    v2 = other_var(wl, 3)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    assert want[0][1]["solved"] > 0
    fill_then_hits(inp, [wl.var, v2], want, 1, opts=SMALL, launches=1, cached=720)
    fill_then_hits(inp, [wl.var, v2], want, 0, opts=SMALL, launches=6, cached=720)


def test_points_without_obs_stay_untouched():
    """Every 25th obs only: points with p = 0 keep their input bits through the merged hits."""
    wl = synth.make("c2", scale=0.1)
    keep = np.arange(wl.obs.shape[0]) % 25 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    inp = Inputs(wl)
    v2 = other_var(wl, 5)
    want = no_reuse(inp, [wl.var, v2])
    assert 0 < want[0][1]["solved"] < wl.points
    untouched = np.all(bits(want[0][0]) == bits(wl.var), axis=0)
    assert untouched.sum() >= wl.points - want[0][1]["solved"]
    fill_then_hits(inp, [wl.var, v2], want, 1, launches=1, cached=wl.points)
    fill_then_hits(inp, [wl.var, v2], want, 0, launches=88, cached=wl.points)


def test_nan_records(monkeypatch):
    """weight_function = 1 (test_gpu_factor_scalars.py's Gaspari-Cohn workload): some points'
    records, factors and step scalars are NaN.  The merged hits carry the same NaN bit
    patterns as the per-batch ones and as the analysis without reuse."""
    core = abi.Core
    monkeypatch.setattr(abi, "Core", lambda *a, **kw: core(*a, weight_function=1, **kw))
    wl = synth.make("c2", nx=13, ny=11, nz=5, k=40, vclr=-1.0, hclr=6.0, n_obs=300)
    inp = Inputs(wl)
    v2 = other_var(wl, 3)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    nan = np.isnan(want[0][0]).any(axis=0)
    assert 0 < nan.sum() < wl.points
    fill_then_hits(inp, [wl.var, v2], want, 1, opts=SMALL, launches=1, cached=wl.points)
    fill_then_hits(inp, [wl.var, v2], want, 0, opts=SMALL, cached=wl.points)


def test_host_slab_takes_the_per_batch_path(w, var2, refs):
    """A pageable host slab that covers its whole grid moves batch by batch beside the solves:
    the call keeps one launch per sub-batch (44 batches of two) whatever the option says."""
    for merge in (1, 0):
        fill_then_hits(Inputs(w), [w.var, var2], refs, merge, host=True, launches=88,
                       cached=w.points)


def test_option_toggling_keeps_the_cache(w, var2, refs):
    """Filled under hit_merge = 1, then 0, then 1 again: the option is no part of the cache's
    key, so every call is still a hit, in the form the option names, with equal bits."""
    r = Run(Inputs(w))
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        same((out, cnt), refs[0])
        for value, launches in ((1, 1), (0, 88), (1, 1)):
            r.c.set_option("hit_merge", value)
            r.c.set_kernel_timing(True)
            for var, ref in ((w.var, refs[0]), (var2, refs[1])):
                out, cnt, info = r.call(var)
                is_hit(info, 44)
                same((out, cnt), ref)
            n, pts = hit_launches(r.c.kernel_times())
            assert (n, pts) == (2 * launches, 2 * w.points), (value, n, pts)
    finally:
        r.close()


def test_option_range():
    c = abi.Core(40, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="ARG"):
                c.set_option("hit_merge", bad)
        c.set_option("hit_merge", 0)
        c.set_option("hit_merge", 1)
    finally:
        c.finalize()
