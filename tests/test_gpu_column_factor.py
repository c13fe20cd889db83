"""GPU tests of CWBL_OPT_COLUMN_FACTOR: a column-shared call (CWBL_OPT_COLUMN_SHARE) on the
one-wavefront path at k = 41..64 and on the hand-off path at k = 65..96 solves every level from
one kept factor per column.  Per (sub-)batch of columns the factor cache's fill kernel
(fill_tq_wave_kernel<KP>, or the hand-off kernel and fill_tqb_tail_kernel<96, 32>) analyses
level 0 on the column view and leaves the factors in a workspace of the call; one launch of
solve_tq_wave_factor_column_kernel<KP> or solve_tqb_factor_column_kernel<96, 32> solves the
levels 1 .. nz-1 from them.

The yardstick of every case is option 0 of CWBL_OPT_COLUMN_SHARE, the per-point call, which
this work does not touch: np.array_equal on the bit patterns of the whole slab and equal
counters (check / analysis of test_gpu_column_share.py, with column_factor = 1 among the
options of every run; the per-point run ignores it).  The fill and the hit kernels are each
bit-identical to the single kernels, and both paths solve one point per wavefront, so there
is no condition on the column count or the quadrature classes.

Workload: test_gpu_column_share.py's, 13 x 11 = 143 columns and nz = 2 (one level in the level
kernel), 9 or 17; `mixed`, `dense`, `trunc` and `straddle` assert their conditions from the
option-0 counters.
"""
import ctypes as C

import numpy as np
import pytest

from cwbl import abi
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits
from test_gpu_column_share import BAD, COLS, INCR_TOL, SEARCH, analysis, check, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FACTOR = (("column_factor", 1),)
BIG = (("big_batch", 64),)  # 143 columns in three sub-batches on the hand-off path


def opts_of(k, more=()):
    return FACTOR + (BIG if k > 64 else ()) + tuple(more)


def kp_of(k):
    return 48 if k <= 48 else 56 if k <= 56 else 64 if k <= 64 else 96


def level_kernel(k):
    kp = kp_of(k)
    return ("solve_tqb_factor_column_kernel<96, 32>" if kp == 96
            else f"solve_tq_wave_factor_column_kernel<{kp}>")


def fill_kernel(k):
    kp = kp_of(k)
    return "fill_tqb_tail_kernel<96, 32>" if kp == 96 else f"fill_tq_wave_kernel<{kp}>"


def auto_levels_per_wave(cols, nl, k):
    """The library's automatic split of the nl = nz - 1 levels above level 0: all of them unless
    the columns (one per wavefront) are fewer than twice the device's resident waves of the
    kernel (3 per SIMD at KP = 48, else 2; 4 SIMDs per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = 2 * cus * 4 * (3 if kp_of(k) == 48 else 2)
    if cols >= want:
        return nl
    ranges = min(nl, -(-want // cols))
    return -(-nl // ranges)


def from_factor(r, k, nz, cols=COLS, launches=None):
    """r ran the fill once per column and the level kernel over the other nz - 1 levels, and no
    group kernel."""
    assert r.info["from_factor"] == 1 and r.info["chunk_launches"] == 0, r.info
    assert r.kt[level_kernel(k)]["points"] == cols * (nz - 1), r.kt
    assert r.kt[fill_kernel(k)]["points"] == cols, r.kt
    assert not [n for n in r.kt if "_multi_kernel<" in n], r.kt
    assert not [n for n in r.kt if n.startswith(("solve_tq_kernel<", "solve_tqb_tail_kernel<"))], r.kt
    if launches is not None:
        assert r.kt[level_kernel(k)]["launches"] == r.kt[fill_kernel(k)]["launches"] == launches
    if k > 64:
        assert r.kt["solve_tq_big_kernel<96, false, 32>"]["points"] == cols, r.kt


# ---- the two paths --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mixed", "dense", "trunc"])
@pytest.mark.parametrize("k", [41, 48, 50, 64])
def test_one_wavefront_path(k, case):
    ref, got = check(k, 9, case, opts=opts_of(k), shares=(1, 2) if k == 64 else (1,))
    for r in got:
        from_factor(r, k, 9, launches=1)
        assert r.info["levels_per_wave"] == auto_levels_per_wave(COLS, 8, k), r.info
    assert ref.info["from_factor"] == 0
    assert level_kernel(k) not in ref.kt and fill_kernel(k) not in ref.kt, ref.kt


@pytest.mark.parametrize("nz", [2, 17])
def test_one_wavefront_path_other_level_counts(nz):
    _, (r,) = check(64, nz, "dense", opts=opts_of(64), shares=(1,))
    from_factor(r, 64, nz)


@pytest.mark.parametrize("case", ["mixed", "dense", "trunc"])
@pytest.mark.parametrize("k", [65, 80, 96])
def test_hand_off_path(k, case):
    """big_batch = 64 splits the batch of 143 columns into three sub-batches, which take turns
    in the workspace."""
    ref, got = check(k, 9, case, opts=opts_of(k), shares=(1, 2) if k == 80 else (1,))
    for r in got:
        from_factor(r, k, 9, launches=3)
    assert ref.info["from_factor"] == 0 and level_kernel(k) not in ref.kt, ref.kt


def test_hand_off_path_two_levels():
    _, (r,) = check(80, 2, "dense", opts=opts_of(80), shares=(1,))
    from_factor(r, 80, 2, launches=3)


# ---- level splits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 80])
def test_level_splits(k):
    """The bits do not depend on the levels per wavefront; the option counts the levels above
    level 0 and is capped by them."""
    nz = 9
    _, got = check(k, nz, "dense", opts=opts_of(k), shares=(1,), levels=(0, 1, 3, nz))
    # the last launch's columns: the batch, or the last sub-batch of 143 = 64 + 64 + 15
    last = 15 if k > 64 else COLS
    for r, lv in zip(got, (0, 1, 3, nz)):
        from_factor(r, k, nz)
        want = min(lv, nz - 1) if lv else auto_levels_per_wave(last, nz - 1, k)
        assert r.info["levels_per_wave"] == want, (lv, r.info)


@pytest.mark.parametrize("k", [64, 80])
def test_mixed_quadrature_classes_are_exact(k):
    _, (r,) = check(k, 9, "straddle", opts=opts_of(k), shares=(1,))
    from_factor(r, k, 9)


# ---- plumbing at k = 50 and k = 80 --------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 80])
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
def test_plumbing(k, variant, case, more):
    ref, got = check(k, 9, case, variant, opts_of(k, more), shares=(1,))
    cols = (12 if variant == "staggered" else 13) * 11
    from_factor(got[0], k, 9, cols=cols)
    if variant == "staggered":  # the last column is not analysed
        for r in [ref] + got:
            assert np.array_equal(bits(r.out[..., -1]), bits(ref.var[..., -1]))
    if variant in ("rtpp", "rtps", "plain", "tune_q"):  # the flags matter
        plain = analysis(k, 9, case, 0, "", 0, opts_of(k))
        assert not np.array_equal(bits(ref.out), bits(plain.out))
    if variant == "tune_q":
        assert got[0].kt["tune_q_kernel"]["points"] == COLS * 9


@pytest.mark.parametrize("k", [64, 80])
def test_gaspari_cohn(k):
    """weight_function = 1: the reference's fp32 Gaspari-Cohn weights give NaN analyses at some
    points; a point's NaN comes from its weights, so it holds at every level of the column."""
    ref, (r,) = check(k, 9, "dense", "gc", opts_of(k), shares=(1,))
    from_factor(r, k, 9)
    nan = np.isnan(ref.out).any(axis=0)  # (nz, ny, nx)
    print(f"gaspari-cohn k={k}: {int(nan[0].sum())} NaN columns of {COLS}")
    assert np.array_equal(nan, np.broadcast_to(nan[0], nan.shape))


@pytest.mark.parametrize("k", [50, 80])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_a_bad_level_stays_in_its_level(k, bad):
    """One member of one level of one column is NaN or Inf: every other level of that column,
    and every other column, equals the clean run."""
    o = opts_of(k)
    clean = analysis(k, 9, "dense", 1, "", 0, o)
    dirty = analysis(k, 9, "dense", 1, bad, 0, o)
    same = analysis(k, 9, "dense", 0, bad, 0, o)
    from_factor(dirty, k, 9)
    assert dirty.cnt == same.cnt == clean.cnt
    assert np.array_equal(bits(dirty.out), bits(same.out))
    _, lev, j, i = BAD
    differs = (bits(dirty.out) != bits(clean.out)).any(axis=0)  # (nz, ny, nx)
    assert differs[lev, j, i]
    assert not np.isfinite(dirty.out[:, lev, j, i]).all()
    differs[lev, j, i] = False
    assert not differs.any(), np.argwhere(differs)


@pytest.mark.parametrize("k", [50, 80])
def test_several_batches_of_columns(k):
    """29 x 23 = 667 columns in search batches of at most 256 with info windows of 256: three
    batches of columns, the window boundaries among them, one workspace for all."""
    o = opts_of(k, (("max_batch", 256), ("info_window", 256)))
    _, (r,) = check(k, 3, "trunc", opts=o, shares=(1,), nx=29, ny=23)
    from_factor(r, k, 3, cols=667)
    assert r.kt[SEARCH]["launches"] == 3, r.kt


# ---- where the option is accepted and ignored -------------------------------------------------------
@pytest.mark.parametrize("k,more", [(16, ()), (32, ()), (32, (("split40", 0),)),
                                    (128, BIG)])
def test_ignored_classes(k, more):
    """k <= 40 and k = 97..128: the shared call runs what it runs without the option."""
    _, (r,) = check(k, 9, "dense", opts=FACTOR + more, shares=(1,))
    off = analysis(k, 9, "dense", 1, "", 0, tuple(more))
    assert r.info == off.info and r.info["from_factor"] == 0, (r.info, off.info)
    assert sorted(r.kt) == sorted(off.kt), (r.kt, off.kt)
    assert {n: t["points"] for n, t in r.kt.items()} == {n: t["points"] for n, t in off.kt.items()}
    assert not [n for n in r.kt if "factor_column" in n or n.startswith("fill_")], r.kt
    assert np.array_equal(bits(r.out), bits(off.out))


@pytest.mark.parametrize("k", [50, 80])
def test_option_off_runs_the_chunks(k):
    """column_factor = 0 (explicitly): the group launches of eight levels, as before."""
    o = (("column_factor", 0),) + (BIG if k > 64 else ())
    _, (r,) = check(k, 9, "dense", opts=o, shares=(1,))
    assert r.info["from_factor"] == 0 and r.info["chunk_launches"] == 2, r.info
    assert [n for n in r.kt if "_multi_kernel<" in n], r.kt
    assert level_kernel(k) not in r.kt and fill_kernel(k) not in r.kt, r.kt


@pytest.mark.parametrize("k", [50, 80])
def test_not_shared(k):
    """column_share = 0, or a 3-D type: the old reasons and the per-point launches."""
    o = dict(opts_of(k))
    w = workload(k, 9, "3d")
    for share, reason in ((0, abi.COLUMN_REASON_OFF), (1, abi.COLUMN_REASON_3D)):
        outs = []
        for factor in (0, 1):
            lib = Lib(w, dict(o, column_share=share, column_factor=factor))
            try:
                lib.c.set_kernel_timing(True)
                outs.append(lib.one(w.var, w.vp) + (lib.c.kernel_times(),))
                info = lib.c.column_info()
                assert info.shared == 0 and info.reason == reason and info.from_factor == 0
            finally:
                lib.close()
        (a, ca, ka), (b, cb, kb) = outs
        assert ca == cb and ca["solved"] > 0 and np.array_equal(bits(a), bits(b))
        assert {n: t["points"] for n, t in ka.items()} == {n: t["points"] for n, t in kb.items()}
        assert not [n for n in kb if "factor_column" in n or n.startswith("fill_")], kb


# ---- the factor caches -------------------------------------------------------------------------------
@pytest.mark.parametrize("k,option", [(50, "wave_reuse"), (80, "big_reuse")])
def test_factor_cache_left_as_it_was(k, option):
    """A per-point call fills the factor cache, a shared column_factor call with other type
    parameters follows, and the first call repeated still solves from the kept factors."""
    w3, w2 = workload(k, 9, "3d"), workload(k, 9, "dense")
    o = dict(opts_of(k), column_share=1)
    o[option] = 1
    lib = Lib(w3, o, reuse_default=True)
    try:
        first, cnt = lib.one(w3.var, w3.vp)
        assert lib.c.column_info().reason == abi.COLUMN_REASON_3D
        fill = lib.c.reuse_info()
        assert fill.batches_assembled > 0 and fill.batches_reused == 0 and fill.bytes_held > 0
        shared, _ = lib.one(w2.var, w2.vp)
        info = lib.c.column_info()
        assert info.shared == 1 and info.from_factor == 1
        mid = lib.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == fill.bytes_held
        assert np.array_equal(bits(shared), bits(analysis(k, 9, "dense", 0, "", 0, opts_of(k)).out))
        again, cnt2 = lib.one(w3.var, w3.vp)
        hit = lib.c.reuse_info()
        assert hit.batches_reused == fill.batches_assembled and hit.batches_assembled == 0
        assert hit.bytes_held == fill.bytes_held
        assert cnt2 == cnt and np.array_equal(bits(again), bits(first))
    finally:
        lib.close()


# ---- against the truth, not only the twin ---------------------------------------------------------
@pytest.mark.parametrize("k", [50, 80])
def test_against_the_oracle(k):
    w = workload(k, 9, "dense")
    r = analysis(k, 9, "dense", 1, "", 0, opts_of(k))
    from_factor(r, k, 9)
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    ref = w.var.copy()
    ost = abi.Stats()
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, w.alt, ref)), 16, C.byref(ost))
    assert rc == 0
    assert r.cnt["solved"] == ost.solved and r.cnt["nobs_sum"] == ost.nobs_sum
    assert r.cnt["max_p"] == ost.max_p
    rel = increment_rel_rms(r.out, ref, w.var)
    moved = np.count_nonzero(bits(ref) != bits(w.var))
    print(f"k={k}: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= INCR_TOL, rel


# ---- arguments ------------------------------------------------------------------------------------------
def test_argument_errors():
    c = abi.Core(50, device=0)
    try:
        for value in (-1, 2):
            with pytest.raises(abi.CwblError, match="CWBL_ERR_ARG"):
                c.set_option("column_factor", value)
        c.set_option("column_factor", 1)
        c.set_option("column_factor", 0)
    finally:
        c.finalize()


def test_init_resets_the_option():
    w = workload(50, 9, "dense")
    lib = Lib(w, {"column_share": 1, "column_factor": 1})
    lib.close()
    lib = Lib(w, {"column_share": 1})
    try:
        lib.one(w.var, w.vp)
        info = lib.c.column_info()
        assert info.shared == 1 and info.from_factor == 0 and info.chunk_launches == 2
    finally:
        lib.close()
