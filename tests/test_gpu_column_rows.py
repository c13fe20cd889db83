"""GPU tests of CWBL_OPT_COLUMN_ROWS: with it the hand-off path at KP = 128 (k = 97..128) is
eligible for CWBL_OPT_COLUMN_FACTOR and CWBL_OPT_COLUMN_REUSE.  Per (sub-)batch of columns the
half-row hand-off kernel and fill_tqb_tail_kernel<128, 64> analyse level 0 on the column view and
leave one BigFactor<128, 64> per column; solve_tqb_factor_column_kernel<128, 64> solves the
levels 1 .. nz-1 from it, and a column-cache hit runs solve_tqb_factor_column_all_kernel
<128, 64> alone.  Without the option (the default) both options stay ignored at these k, which
test_gpu_column_factor.py and test_gpu_column_reuse.py pin and the last section here restates.

The yardstick of every comparison is the same call on a fresh core with column_share = 0, the
per-point call, which this work does not touch: np.array_equal on the bit patterns of the whole
slab and equal counters.  A level is the half-row hit's body, bit-identical to the kernel pair,
and every kernel solves one point per wavefront, so there is no tolerance anywhere except
against the oracle (INCR_TOL, the project's bar).

Workload: test_gpu_column_share.py's, 13 x 11 = 143 columns with big_batch = 64, so that three
sub-batches (64 + 64 + 15 columns) take turns in the workspace; k = 127 and 112 exercise the
steps that the select drops and the padding rows of members 64 + l >= k.
"""
import ctypes as C
import math

import numpy as np
import pytest

from cwbl import abi
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, other_var
from test_gpu_column_reuse import Seq, same, shift_x, var_of, yard
from test_gpu_column_share import BAD, COLS, INCR_TOL, NX, NY, SEARCH, analysis, check, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HANDOFF = "solve_tq_rows_kernel<128, 64>"
FILL = "fill_tqb_tail_kernel<128, 64>"
LEVEL = "solve_tqb_factor_column_kernel<128, 64>"
ALL = "solve_tqb_factor_column_all_kernel<128, 64>"
HIT = "solve_tqb_factor_kernel<128, 64>"
BIG = (("big_batch", 64),)
ROWS = (("column_rows", 1),)
FACTOR = ROWS + (("column_factor", 1),) + BIG
POINT = (("column_share", 0),) + BIG     # the yardstick of the column cache's sequences
BUDGET = 64                              # MiB: every column of these workloads fits
COLUMN_BYTES = 8705 * 8                  # BigFactor<128, 64>
KS = (97, 112, 127, 128)


def points(kt):
    return {n: t["points"] for n, t in kt.items()}


def auto_levels_per_wave(cols, nl):
    """The library's automatic split of nl levels over `cols` columns, one per wavefront: all of
    them unless the columns are fewer than twice the device's resident waves of the kernel, two
    per SIMD and four SIMDs per CU; then the fewest level ranges that reach that many."""
    want = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4 * 2
    if cols >= want:
        return nl
    ranges = min(nl, -(-want // cols))
    return -(-nl // ranges)


def from_factor(r, nz, cols=COLS, launches=None):
    """r ran the hand-off kernel and the fill once per column, the level kernel over the other
    nz - 1 levels, the searches (the tree's kernel is in the table of every binned call) and
    nothing else."""
    assert r.info["from_factor"] == 1 and r.info["chunk_launches"] == 0, r.info
    solves = sorted(n for n in r.kt if not n.startswith("search_") and n != "tune_q_kernel")
    assert solves == sorted([HANDOFF, FILL, LEVEL]), r.kt
    assert r.kt[HANDOFF]["points"] == r.kt[FILL]["points"] == cols, r.kt
    assert r.kt[LEVEL]["points"] == cols * (nz - 1), r.kt
    assert not [n for n in r.kt if "_multi_kernel<" in n or n.startswith("solve_tqb_tail_kernel<")]
    assert r.kt[SEARCH]["points"] == cols, r.kt  # the fourth kernel: one search lane per column
    if launches is not None:
        assert r.kt[LEVEL]["launches"] == r.kt[FILL]["launches"] == launches, r.kt


# ---- column factor -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [2, 9, 17])
@pytest.mark.parametrize("case", ["mixed", "dense", "trunc"])
@pytest.mark.parametrize("k", KS)
def test_every_level_from_one_factor(k, case, nz):
    ref, got = check(k, nz, case, opts=FACTOR, shares=(1, 2))
    for r in got:
        from_factor(r, nz, launches=3)
        # (the last launch's: the sub-batch of 15 columns)
        assert r.info["levels_per_wave"] == auto_levels_per_wave(15, nz - 1), r.info
    assert ref.info["from_factor"] == 0
    assert LEVEL not in ref.kt and FILL not in ref.kt and HANDOFF in ref.kt, ref.kt


@pytest.mark.parametrize("k", [97, 128])
def test_level_splits(k):
    """The bits do not depend on the levels per wavefront; the option counts the levels above
    level 0 and is capped by them."""
    nz = 9
    _, got = check(k, nz, "dense", opts=FACTOR, shares=(1,), levels=(0, 1, 3, nz - 1))
    for r, lv in zip(got, (0, 1, 3, nz - 1)):
        from_factor(r, nz, launches=3)
        assert r.info["levels_per_wave"] == (lv or auto_levels_per_wave(15, nz - 1)), (lv, r.info)


def test_automatic_split_counts_two_waves_per_simd():
    """667 columns in one sub-batch and 16 levels above level 0: on a device of 256 compute
    units two waves per SIMD give 7 ranges of 3 levels, three would give 10 of 2."""
    o = ROWS + (("column_factor", 1),)
    _, (r,) = check(128, 17, "trunc", opts=o, shares=(1,), nx=29, ny=23)
    from_factor(r, 17, cols=667, launches=1)
    assert r.info["levels_per_wave"] == auto_levels_per_wave(667, 16), r.info


def test_several_batches_of_columns():
    """29 x 23 = 667 columns in search batches of at most 256 with info windows of 256: three
    batches of columns, the window boundaries among them, one workspace for all."""
    o = FACTOR + (("max_batch", 256), ("info_window", 256))
    _, (r,) = check(128, 3, "trunc", opts=o, shares=(1,), nx=29, ny=23)
    from_factor(r, 3, cols=667)
    assert r.kt[SEARCH]["launches"] == 3, r.kt


@pytest.mark.parametrize("variant,case,more", [
    ("staggered", "mixed", ()),
    ("pageable", "mixed", ()),
    ("pinned", "mixed", ()),
    ("pageable", "dense", (("host_pipe", 1),)),
    ("pinned", "dense", (("host_pipe", 1),)),
    ("", "mixed", (("index", 1),)),
    ("", "trunc", (("index", 1),)),
    ("rtpp", "dense", ()),
    ("rtps", "dense", ()),
    ("plain", "dense", ()),
    ("tune_q", "mixed", ()),
    ("tune_q", "dense", ()),
])
def test_plumbing(variant, case, more):
    k = 112
    ref, got = check(k, 9, case, variant, FACTOR + tuple(more), shares=(1,))
    cols = (12 if variant == "staggered" else 13) * 11
    from_factor(got[0], 9, cols=cols)
    if variant == "staggered":  # the last column is not analysed
        for r in [ref] + got:
            assert np.array_equal(bits(r.out[..., -1]), bits(ref.var[..., -1]))
    if variant in ("rtpp", "rtps", "plain", "tune_q"):  # the flags matter
        plain = analysis(k, 9, case, 0, "", 0, FACTOR)
        assert not np.array_equal(bits(ref.out), bits(plain.out))
    if variant == "tune_q":
        assert got[0].kt["tune_q_kernel"]["points"] == COLS * 9


def test_gaspari_cohn():
    """weight_function = 1: the reference's fp32 Gaspari-Cohn weights give NaN analyses at some
    points; a point's NaN comes from its weights, so it holds at every level of the column."""
    ref, (r,) = check(128, 9, "dense", "gc", FACTOR, shares=(1,))
    from_factor(r, 9)
    nan = np.isnan(ref.out).any(axis=0)  # (nz, ny, nx)
    print(f"gaspari-cohn k=128: {int(nan[0].sum())} NaN columns of {COLS}")
    assert np.array_equal(nan, np.broadcast_to(nan[0], nan.shape))


@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_a_bad_level_stays_in_its_level(bad):
    """One member of one level of one column is NaN or Inf: every other level of that column,
    and every other column, equals the clean run."""
    k = 112
    clean = analysis(k, 9, "dense", 1, "", 0, FACTOR)
    dirty = analysis(k, 9, "dense", 1, bad, 0, FACTOR)
    point = analysis(k, 9, "dense", 0, bad, 0, FACTOR)
    from_factor(dirty, 9)
    assert dirty.cnt == point.cnt == clean.cnt
    assert np.array_equal(bits(dirty.out), bits(point.out))
    _, lev, j, i = BAD
    differs = (bits(dirty.out) != bits(clean.out)).any(axis=0)  # (nz, ny, nx)
    assert differs[lev, j, i]
    assert not np.isfinite(dirty.out[:, lev, j, i]).all()
    differs[lev, j, i] = False
    assert not differs.any(), np.argwhere(differs)


# ---- column cache ------------------------------------------------------------------------------------
def reuse_opts(more=(), budget=BUDGET):
    return (("column_share", 1),) + FACTOR + (("column_reuse", budget),) + tuple(more)


def pt(k, case, nz, variant="", opts=POINT, **kw):
    """The arguments of the per-point yardstick (yard of test_gpu_column_reuse.py)."""
    return (k, case, nz, variant, opts), kw


def same_point(r, k, case, nz, variant="", **kw):
    args, kw = pt(k, case, nz, variant, **kw)
    ref = yard(*args, **kw)
    assert ref.info["shared"] == 0 and ref.info["reason"] == abi.COLUMN_REASON_OFF, ref.info
    same(r, ref)
    return r


def is_fill(r, nz, cols=COLS):
    """r searched and assembled per column, and left every column in the cache."""
    assert r.info["shared"] == 1 and r.info["levels"] == nz and r.info["columns"] == cols, r.info
    assert r.info["from_factor"] == 1 and r.info["chunk_launches"] == 0, r.info
    assert r.reuse["columns_filled"] == cols and r.reuse["columns_reused"] == 0, r.reuse
    assert r.reuse["batches_reused"] == 0 and r.reuse["form"] == abi.COLUMN_FORM_BIG, r.reuse
    assert r.reuse["bytes_held"] >= cols * COLUMN_BYTES, r.reuse
    assert r.kt[SEARCH]["points"] == cols, r.kt
    assert r.kt[HANDOFF]["points"] == r.kt[FILL]["points"] == cols and ALL not in r.kt, r.kt
    if nz > 1:
        assert r.kt[LEVEL]["points"] == cols * (nz - 1), r.kt
    else:
        assert LEVEL not in r.kt, r.kt
    assert not [n for n in r.kt if "_multi_kernel<" in n or n.startswith("solve_tqb_tail_")], r.kt
    return r


def is_hit(r, nz, cols=COLS):
    """r solved every level of every column from the cache, in launches of the all-levels kernel
    alone (tune_q aside), with no obs preparation, tree or bin work."""
    assert r.info["shared"] == 1 and r.info["levels"] == nz and r.info["columns"] == cols, r.info
    assert r.info["from_factor"] == 1 and r.info["chunk_launches"] == 0, r.info
    assert r.reuse["columns_reused"] == cols and r.reuse["columns_filled"] == 0, r.reuse
    assert r.reuse["batches_reused"] >= 1 and r.reuse["form"] == abi.COLUMN_FORM_BIG, r.reuse
    assert r.reuse["ms_compare"] > 0.0, r.reuse
    assert sorted(n for n in r.kt if n != "tune_q_kernel") == [ALL], r.kt
    assert r.kt[ALL]["points"] == cols * nz, r.kt
    assert r.prep["trees_built"] == r.prep["bins_built"] == 0, r.prep
    assert r.prep["ms_columns"] == 0.0 and r.prep["ms_bins"] == 0.0, r.prep
    return r


@pytest.mark.parametrize("case", ["dense", "mixed"])
@pytest.mark.parametrize("k", [97, 128])
def test_sequence(k, case):
    """MU -> P -> PH: nz = 1 fills, nz = 9 and nz = 10 (each with an alt of its own) hit; every
    slab is the per-point call's."""
    s = Seq(k, case, reuse_opts())
    try:
        got = [s.call(nz) for nz in (1, 9, 10)]
    finally:
        s.close()
    is_fill(got[0], 1)
    assert got[0].info["levels_per_wave"] == 0, got[0].info
    for r, nz in zip(got[1:], (9, 10)):
        is_hit(r, nz)
        assert r.kt[ALL]["launches"] == 3, r.kt
        assert r.info["levels_per_wave"] == auto_levels_per_wave(15, nz), r.info
        assert r.reuse["bytes_held"] == got[0].reuse["bytes_held"]
    for r, nz in zip(got, (1, 9, 10)):
        same_point(r, k, case, nz)
    ref = yard(*pt(k, case, 9)[0])
    assert not np.array_equal(bits(ref.out), bits(var_of(s.w, "", 9)))  # something was analysed
    if case == "mixed":
        assert 0 < ref.cnt["solved"] < ref.cnt["points"]


def test_misses_refill():
    k = 128
    s = Seq(k, "dense", reuse_opts())

    def yardstick(r, nz, variant="", **kw):
        """r is compared with the per-point call when the core is closed."""
        return s.same(r, *pt(k, "dense", nz, variant)[0], **kw)

    try:
        is_fill(s.call(1), 1)
        is_hit(s.call(9), 9)
        # another hclr, another multi_infl: other keys
        for variant in ("hclr", "infl"):
            is_fill(yardstick(s.call(9, variant), 9, variant), 9)
            is_hit(yardstick(s.call(10, variant), 10, variant), 10)
        # the obs set again
        is_fill(s.call(9), 9)
        s.lib.c.set_obs(abi.ObsSetBuilder().add_radar(s.w.radar_type, s.w.obs_xyz, s.w.obs,
                                                      s.w.hdxb).build())
        is_fill(yardstick(s.call(9), 9), 9)
        # an option
        is_hit(s.call(10), 10)
        s.lib.c.set_option("info_window", 512)
        is_fill(yardstick(s.call(10), 10), 10)
        # ix_lim: the staggered slab, 12 x 11 columns
        cols = (NX - 1) * NY
        r = is_fill(yardstick(s.call(9, "staggered"), 9, "staggered"), 9, cols)
        is_hit(yardstick(s.call(10, "staggered"), 10, "staggered"), 10, cols)
        assert np.array_equal(bits(r.out[..., -1]), bits(var_of(s.w, "", 9)[..., -1]))
        # x rewritten in place behind an equal key
        is_fill(s.call(9), 9)
        shift_x(s)
        r = is_fill(yardstick(s.call(9), 9, xshift=True), 9)
        assert r.reuse["ms_compare"] > 0.0
        is_hit(yardstick(s.call(1), 1, xshift=True), 1)
    finally:
        s.close()


def test_a_3d_call_in_between_leaves_the_cache():
    k = 128
    s = Seq(k, "dense", reuse_opts())
    try:
        is_fill(s.call(1), 1)
        held = s.call(9).reuse["bytes_held"]
        r = s.call(9, "3d")
        assert r.info["shared"] == 0 and r.info["reason"] == abi.COLUMN_REASON_3D, r.info
        assert r.reuse["columns_reused"] == r.reuse["columns_filled"] == 0, r.reuse
        assert r.reuse["bytes_held"] == held
        assert HANDOFF in r.kt and "solve_tqb_tail_kernel<128, 64, 3>" in r.kt, r.kt
        s.same(r, *pt(k, "dense", 9, "3d")[0])
        is_hit(s.same(s.call(10), *pt(k, "dense", 10)[0]), 10)
    finally:
        s.close()


def test_a_hit_split_otherwise_than_its_fill():
    k = 128
    s = Seq(k, "dense", reuse_opts((("column_levels", 3),)))
    try:
        r = is_fill(s.same(s.call(9), *pt(k, "dense", 9)[0]), 9)
        assert r.info["levels_per_wave"] == 3, r.info
        for lv in (1, 4, 10):
            s.lib.c.set_option("column_levels", lv)
            r = is_hit(s.same(s.call(10), *pt(k, "dense", 10)[0]), 10)
            assert r.info["levels_per_wave"] == lv, r.info
    finally:
        s.close()


def three_batches(budget):
    return reuse_opts((("max_batch", 256), ("info_window", 256)), budget)


POINT3 = POINT + (("max_batch", 256), ("info_window", 256))


def test_partial_budget():
    """29 x 23 = 667 columns in batches of 256, 256 and 155: a budget that holds the first
    batch's 256 + 1 entries and not the second's."""
    k = 128
    budget = math.ceil(257 * COLUMN_BYTES / 2 ** 20)
    assert 257 * COLUMN_BYTES <= budget * 2 ** 20 < 2 * 257 * COLUMN_BYTES
    s = Seq(k, "trunc", three_batches(budget), 29, 23)
    try:
        a, b = s.call(1), s.call(3)
    finally:
        s.close()
    assert a.reuse["columns_filled"] == 256 and a.reuse["batches_reused"] == 0, a.reuse
    assert a.kt[SEARCH]["launches"] == 3, a.kt
    assert b.reuse["columns_reused"] == 256 and b.reuse["batches_reused"] == 1, b.reuse
    assert b.kt[ALL]["points"] == 256 * 3, b.kt
    assert b.kt[SEARCH]["launches"] == 2 and b.kt[SEARCH]["points"] == 667 - 256, b.kt
    assert b.kt[FILL]["points"] == b.kt[HANDOFF]["points"] == 667 - 256, b.kt
    assert b.kt[LEVEL]["points"] == (667 - 256) * 2, b.kt
    same(a, yard(k, "trunc", 1, "", POINT3, 29, 23))
    same(b, yard(k, "trunc", 3, "", POINT3, 29, 23))


def test_every_batch_cached():
    k = 128
    s = Seq(k, "trunc", three_batches(BUDGET), 29, 23)
    try:
        a, b = s.call(3), s.call(1)
    finally:
        s.close()
    is_fill(a, 3, 667)
    is_hit(b, 1, 667)
    assert b.reuse["batches_reused"] == 3
    same(a, yard(k, "trunc", 3, "", POINT3, 29, 23))
    same(b, yard(k, "trunc", 1, "", POINT3, 29, 23))


def test_no_budget_runs_as_without_the_option():
    """A budget below one batch's need: nothing is held and column_factor's workspace serves."""
    k = 128
    o = three_batches(1)
    base = tuple((n, v) for n, v in o if n != "column_reuse")
    ref = yard(k, "trunc", 3, "", base, 29, 23)
    s = Seq(k, "trunc", o, 29, 23)
    try:
        for _ in range(2):
            r = s.call(3)
            assert r.reuse["bytes_held"] == 0 and r.reuse["form"] == abi.COLUMN_FORM_NONE, r.reuse
            assert r.reuse["columns_filled"] == r.reuse["columns_reused"] == 0, r.reuse
            same(r, ref)
            assert points(r.kt) == points(ref.kt)
            assert r.kt[LEVEL]["points"] == 667 * 2 and ALL not in r.kt, r.kt
    finally:
        s.close()
    same(ref, yard(k, "trunc", 3, "", POINT3, 29, 23))


# ---- where nothing changes ------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [None, 0])
def test_without_the_option_both_options_stay_ignored(rows):
    """column_rows = 0 (the default, or set): at k = 128 a call with column_factor and
    column_reuse set launches what the call without them launches."""
    k = 128
    both = (("column_share", 1), ("column_factor", 1)) + BIG
    if rows is not None:
        both += (("column_rows", rows),)
    s = Seq(k, "dense", both + (("column_reuse", BUDGET),))
    try:
        got = [s.call(nz) for nz in (9, 9, 1)]
    finally:
        s.close()
    for r, nz in zip(got, (9, 9, 1)):
        ref = yard(k, "dense", nz, "", (("column_share", 1),) + BIG)
        same(r, ref)
        assert r.info == ref.info and r.info["from_factor"] == 0, (r.info, ref.info)
        assert r.reuse == ref.reuse and r.reuse["bytes_held"] == 0, r.reuse
        assert points(r.kt) == points(ref.kt), (r.kt, ref.kt)
        assert not [n for n in r.kt if "factor_column" in n or n.startswith("fill_")], r.kt
    assert got[0].info["chunk_launches"] == 2 and got[2].info["reason"] == abi.COLUMN_REASON_NZ


def test_the_option_alone_runs_the_chunks():
    o = ROWS + (("column_factor", 0), ("column_reuse", 0)) + BIG
    _, (r,) = check(128, 9, "dense", opts=o, shares=(1,))
    off = analysis(128, 9, "dense", 1, "", 0, BIG)
    assert r.info == off.info and r.info["from_factor"] == 0 and r.info["chunk_launches"] == 2
    assert points(r.kt) == points(off.kt), (r.kt, off.kt)
    assert [n for n in r.kt if "_multi_kernel<" in n], r.kt
    assert not [n for n in r.kt if "factor_column" in n or n.startswith("fill_")], r.kt


@pytest.mark.parametrize("k", [80, 50, 32])
def test_ignored_at_the_smaller_sizes(k):
    """k <= 96: the shared call under column_factor is the one without column_rows."""
    more = (("column_factor", 1),) + (BIG if k > 64 else ())
    _, (r,) = check(k, 9, "dense", opts=ROWS + more, shares=(1,))
    off = analysis(k, 9, "dense", 1, "", 0, more)
    assert r.info == off.info, (r.info, off.info)
    assert points(r.kt) == points(off.kt), (r.kt, off.kt)
    assert np.array_equal(bits(r.out), bits(off.out))


@pytest.mark.parametrize("more", [(("big_path", 0),), ()])
def test_ignored_off_the_hand_off_path_and_for_groups(more):
    k = 128
    w = workload(k, 3, "dense")
    if more:  # one 256-thread kernel per point: no path of a shared call, with or without it
        on = analysis(k, 3, "dense", 1, "", 0, ROWS + (("column_factor", 1),) + more)
        off = analysis(k, 3, "dense", 1, "", 0, more)
        assert on.info == off.info and on.info["shared"] == 0, (on.info, off.info)
        assert on.info["reason"] == abi.COLUMN_REASON_PATH, on.info
        assert points(on.kt) == points(off.kt), (on.kt, off.kt)
        assert on.cnt == off.cnt and np.array_equal(bits(on.out), bits(off.out))
        return
    outs = []
    for rows in (0, 1):
        lib = Lib(w, dict(FACTOR, column_share=1, column_rows=rows, column_reuse=BUDGET))
        try:
            outs.append(lib.group([w.var, other_var(w, 7)], [w.vp] * 2))
            info, reuse = lib.c.column_info(), lib.c.column_reuse_info()
            assert info.shared == 0 and info.reason == abi.COLUMN_REASON_GROUP
            assert reuse.columns_filled == reuse.columns_reused == reuse.bytes_held == 0
        finally:
            lib.close()
    (a, ca), (b, cb) = outs
    assert ca == cb and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_not_shared():
    """column_share = 0, or a 3-D type: the old reasons and the per-point launches."""
    k = 128
    w = workload(k, 9, "3d")
    for share, reason in ((0, abi.COLUMN_REASON_OFF), (1, abi.COLUMN_REASON_3D)):
        outs = []
        for rows in (0, 1):
            lib = Lib(w, dict(BIG, column_share=share, column_factor=rows, column_rows=rows,
                              column_reuse=BUDGET * rows))
            try:
                lib.c.set_kernel_timing(True)
                outs.append(lib.one(w.var, w.vp) + (lib.c.kernel_times(),))
                info = lib.c.column_info()
                assert info.shared == 0 and info.reason == reason and info.from_factor == 0
                assert lib.c.column_reuse_info().bytes_held == 0
            finally:
                lib.close()
        (a, ca, ka), (b, cb, kb) = outs
        assert ca == cb and ca["solved"] > 0 and np.array_equal(bits(a), bits(b))
        assert points(ka) == points(kb)
        assert not [n for n in kb if "factor_column" in n or n.startswith("fill_")], kb


def test_rows_reuse_cache_left_as_it_was():
    """A per-point call fills the factor cache of rows_reuse, a shared call and a column-cache
    sequence follow, and the first call repeated still solves from the kept factors; the column
    cache still serves after it."""
    k = 128
    o = dict(reuse_opts(), rows_reuse=1)
    s = Seq(k, "dense", o, record_reuse=True)
    try:
        first = s.same(s.call(9, "3d"), *pt(k, "dense", 9, "3d")[0])
        fill = s.lib.c.reuse_info()
        assert fill.batches_assembled > 0 and fill.batches_reused == 0 and fill.bytes_held > 0
        assert FILL in first.kt, first.kt
        is_fill(s.call(1), 1)
        is_hit(s.call(9), 9)
        mid = s.lib.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == fill.bytes_held
        again = s.call(9, "3d")
        hit = s.lib.c.reuse_info()
        assert hit.batches_reused == fill.batches_assembled and hit.batches_assembled == 0
        assert hit.bytes_held == fill.bytes_held
        assert sorted(again.kt) == [HIT], again.kt
        assert again.reuse["columns_reused"] == 0
        same(again, first)
        is_hit(s.call(10), 10)
    finally:
        s.close()


# ---- arguments ------------------------------------------------------------------------------------------
def test_argument_errors_and_init():
    c = abi.Core(128, device=0)
    try:
        for value in (2, -1):
            with pytest.raises(abi.CwblError, match="CWBL_ERR_ARG"):
                c.set_option("column_rows", value)
        c.set_option("column_rows", 1)
        c.set_option("column_rows", 0)
    finally:
        c.finalize()
    # cwbl_init resets the option
    w = workload(128, 9, "dense")
    lib = Lib(w, dict(FACTOR, column_share=1))
    lib.close()
    lib = Lib(w, dict(BIG, column_share=1, column_factor=1))
    try:
        lib.one(w.var, w.vp)
        info = lib.c.column_info()
        assert info.shared == 1 and info.from_factor == 0 and info.chunk_launches == 2
    finally:
        lib.close()


# ---- against the truth, not only the twin ---------------------------------------------------------
def oracle_run(w, var, alt):
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    ref = var.copy()
    ost = abi.Stats()
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, alt, ref)), 16, C.byref(ost))
    assert rc == 0
    return ref, ost


def against(r, ref, ost, var, what):
    assert r.cnt["solved"] == ost.solved and r.cnt["nobs_sum"] == ost.nobs_sum
    assert r.cnt["max_p"] == ost.max_p
    rel = increment_rel_rms(r.out, ref, var)
    moved = np.count_nonzero(bits(ref) != bits(var))
    print(f"k=128 {what}: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= INCR_TOL, rel


def test_against_the_oracle_from_the_workspace():
    w = workload(128, 3, "dense")
    r = analysis(128, 3, "dense", 1, "", 0, FACTOR)
    from_factor(r, 3)
    ref, ost = oracle_run(w, w.var, w.alt)
    against(r, ref, ost, w.var, "from the workspace")


def test_against_the_oracle_on_a_hit():
    s = Seq(128, "dense", reuse_opts())
    try:
        is_fill(s.call(1), 1)
        r = is_hit(s.call(3), 3)
    finally:
        s.close()
    w = s.w
    var = var_of(w, "", 3)
    ref, ost = oracle_run(w, var, np.ascontiguousarray(w.alt[:3] + np.float32(21.0)))
    against(r, ref, ost, var, "a column-cache hit")
