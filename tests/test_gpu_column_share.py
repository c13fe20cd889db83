"""GPU tests of CWBL_OPT_COLUMN_SHARE: a variable whose obs types all localise in 2-D (vclr <= 0)
analysed once per column.  The neighbour lists, A, b1, the tridiagonal factor, the quadrature
level and info of a point then depend on its column only, so the call searches, assembles and
tridiagonalises per column and solves every level from that factor: solve_tq40_column_kernel on
the k = 17..40 record path (option 1), the group kernels over chunks of up to eight levels on
the one-wavefront and hand-off paths (option 1) and on the record path too (option 2).

The yardstick of every case is the same call with option 0, the per-point path this work
leaves as it was: np.array_equal on the bit patterns of the whole slab and equal counters.

One condition bounds that on the record path.  Its kernels solve four points per wavefront
under the quadrature rule of the wave's largest round class (15 nodes up to a spectrum bound
M/m of 1e3, 23 up to 1e5, ...).  Option 0's waves hold the points 4n .. 4n + 3 of the slab, a
shared call's the columns 4n .. 4n + 3 at every level: the same sets only when the column count
is a multiple of 4.  On 143 columns the bit comparison therefore holds as long as no wave mixes
classes, which is so for `mixed`, `dense` and `trunc` (every point in the 15-node class;
conditions() asserts it from the counters).  `straddle` (obs error 0.7: M/m from ~400 to ~1400
over the columns) mixes them: there the comparison is exact on 12 x 11 = 132 columns, and on 143
columns options 1 and 2 equal each other exactly, for every split, and meet the project's
path-versus-oracle bar INCR_TOL against option 0 and against the oracle (the rules agree to
~1e-12 relative, the bar is the fp32 analysis's).  The one-wavefront and hand-off kernels solve
one point per wavefront: exact there on 143 columns too.

Workload: synth c2 with vclr = -1 on 13 x 11 columns (143: no multiple of 4 or 64) and nz = 2,
9 or 17 levels (chunks of 2, 8 + 1, 8 + 8 + 1); `mixed` has empty columns and sparse p < k ones,
`dense` reaches p >= k, `trunc` passes max_lz_pts (the tree re-search on the column view).
Each case asserts these conditions from the option-0 counters.
"""
import collections
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, counters, other_var, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INCR_TOL = 1e-6
NX, NY = 13, 11
COLS = NX * NY
CASES = {"mixed": dict(hclr=0.8, n_obs=60, max_lz=1000),
         "dense": dict(hclr=6.0, n_obs=300, max_lz=1000),
         "trunc": dict(hclr=6.0, n_obs=300, max_lz=24),
         "straddle": dict(hclr=6.0, n_obs=300, max_lz=1000, err=0.7),
         "3d": dict(hclr=6.0, n_obs=300, max_lz=1000, vclr=3.0)}
COLUMN = "solve_tq40_column_kernel<40>"
MULTI = "solve_tq40_multi_kernel<40>"
SINGLE40 = "solve_tq40_kernel<40, 0>"
ASSEMBLE = "assemble_record_kernel<4>"
SEARCH = "search_binned_kernel"

Res = collections.namedtuple("Res", "out cnt info kt var")


@functools.lru_cache(maxsize=None)
def workload(k, nz, case, nx=NX, ny=NY):
    kw = dict(vclr=-1.0)
    kw.update(CASES[case])
    return synth.make("c2", nx=nx, ny=ny, nz=nz, k=k, **kw)


def vp_of(w, variant):
    vp = copy.deepcopy(w.vp)
    if variant == "rtpp":
        vp.use_rtps = 0
    elif variant == "rtps":
        vp.use_rtpp = 0
    elif variant == "plain":
        vp.use_rtpp = vp.use_rtps = 0
    elif variant == "tune_q":
        vp.tune_q = 1
    return vp


BAD = (5, 4, 6, 7)  # member, level, row, column of the isolation cases' bad value


def var_of(w, variant):
    if variant in ("nan", "inf"):
        var = w.var.copy()
        var[BAD] = np.nan if variant == "nan" else np.inf
        return var
    return w.var


@functools.lru_cache(maxsize=None)
def analysis(k, nz, case, share, variant="", levels=0, opts=(), nx=NX, ny=NY):
    """One cwbl_analyze_var on a fresh core under column_share = share: the analysis, the
    counters, column_info and the kernel times.  Computed once per argument set; shared."""
    w = workload(k, nz, case, nx, ny)
    o = dict(opts)
    o["column_share"] = share
    if levels:
        o["column_levels"] = levels
    host = variant in ("pageable", "pinned")
    lib = Lib(w, o, host=host, weight_function=1 if variant == "gc" else 0)
    try:
        lib.c.set_kernel_timing(True)
        var, vp = var_of(w, variant), vp_of(w, variant)
        ix_lim = alt = keep = None
        if variant == "staggered":  # ix_lim < nx and an alt array narrower than var
            ix_lim = w.nx - 1
            alt = to_dev(w.alt[:, :, :ix_lim])
        if variant == "pinned":
            keep = torch.empty(var.shape, dtype=torch.float32).pin_memory()
            buf = keep.numpy()
            buf[...] = var
        else:
            buf, = lib.buffers([var])
        st = lib.c.analyze_var(vp, lib.slab(buf, ix_lim, alt=alt))
        out = np.array(lib.fetch(buf), copy=True)
        return Res(out, counters(st), lib.c.column_info().as_dict(), lib.c.kernel_times(), var)
    finally:
        lib.close()


def conditions(case, cnt, k):
    """The input conditions of a case, from the option-0 run's counters."""
    print(f"{case} k={k}: {cnt}")
    assert cnt["solved"] > 0
    if case == "mixed":
        assert 0 < cnt["solved"] < cnt["points"]
        assert cnt["nobs_sum"] / cnt["solved"] < k  # sparse: p < k on average
    if case == "dense":
        assert cnt["max_p"] >= k
    if case == "trunc":
        assert cnt["lz_truncated"] > 0
    # quadrature levels (sweeps) on both sides of the 15- / 23-node boundary, or on one side
    if case == "straddle":
        assert cnt["max_sweeps"] >= 4 and cnt["sweeps_sum"] < 4 * cnt["solved"]
        assert cnt["max_sweeps"] <= 5
    else:
        assert cnt["max_sweeps"] <= 3  # one round class: no wave of four mixes classes


def auto_levels_per_wave(cols, nz):
    """The library's automatic split: all levels unless the columns' waves are fewer than twice
    the device's resident waves of the kernel (2 per SIMD, 4 SIMDs per CU)."""
    waves, want = (cols + 3) // 4, 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8
    if waves >= want:
        return nz
    ranges = min(nz, -(-want // waves))
    return -(-nz // ranges)


def check(k, nz, case="mixed", variant="", opts=(), shares=(1, 2), levels=(0,), nx=NX, ny=NY):
    """Options `shares` against option 0: bit-equal slabs, equal counters, shared per column."""
    ref = analysis(k, nz, case, 0, variant, 0, opts, nx, ny)
    conditions(case, ref.cnt, k)
    assert ref.info["shared"] == 0 and ref.info["reason"] == abi.COLUMN_REASON_OFF
    assert not np.array_equal(bits(ref.out), bits(ref.var))  # the call analysed something
    cols = (nx - 1 if variant == "staggered" else nx) * ny
    assert ref.cnt["points"] == cols * nz
    got = []
    for share in shares:
        for lv in levels:
            r = analysis(k, nz, case, share, variant, lv, opts, nx, ny)
            assert r.cnt == ref.cnt, (share, lv, r.cnt, ref.cnt)
            assert np.array_equal(bits(r.out), bits(ref.out)), (share, lv)
            assert r.info["shared"] == 1 and r.info["reason"] == abi.COLUMN_SHARED, r.info
            assert r.info["columns"] == cols and r.info["levels"] == nz, r.info
            assert r.kt[SEARCH]["points"] == cols, r.kt  # one search lane per column
            got.append(r)
    return ref, got


# ---- record path -------------------------------------------------------------------------------
RECORD = [(32, 9, "mixed"), (32, 9, "dense"), (32, 9, "trunc"), (32, 2, "dense"),
          (32, 17, "mixed"), (17, 9, "dense"), (17, 2, "mixed"), (17, 17, "trunc"),
          (40, 9, "mixed"), (40, 17, "dense"), (40, 2, "trunc")]


@pytest.mark.parametrize("k,nz,case", RECORD)
def test_record_path_column_kernel(k, nz, case):
    """Option 1: the column kernel, at 1, 3 and nz levels per wave and the automatic split."""
    ref, got = check(k, nz, case, shares=(1,), levels=(0, 1, 3, nz))
    for r, lv in zip(got, (0, 1, 3, nz)):
        want = min(lv, nz) if lv else auto_levels_per_wave(COLS, nz)
        assert r.info["levels_per_wave"] == want, r.info
        assert r.info["chunk_launches"] == 0
        assert r.kt[COLUMN]["points"] == COLS * nz, r.kt
        assert r.kt[ASSEMBLE]["points"] == COLS, r.kt  # one record per column
        assert MULTI not in r.kt and SINGLE40 not in r.kt, r.kt
    assert SINGLE40 in ref.kt and COLUMN not in ref.kt, ref.kt
    assert ref.kt[ASSEMBLE]["points"] == COLS * nz, ref.kt


@pytest.mark.parametrize("k,nz,case", RECORD)
def test_record_path_level_chunks(k, nz, case):
    """Option 2: solve_tq40_multi_kernel per chunk of eight levels, the single kernel for a
    remainder of one, all on one assembly per column."""
    _, (r,) = check(k, nz, case, shares=(2,))
    assert r.info["chunk_launches"] == (nz + 7) // 8 and r.info["levels_per_wave"] == 0, r.info
    assert COLUMN not in r.kt, r.kt
    assert r.kt[ASSEMBLE]["points"] == COLS, r.kt
    assert r.kt[MULTI]["points"] == COLS * (nz - nz % 8 if nz % 8 == 1 else nz), r.kt
    assert (SINGLE40 in r.kt) == (nz % 8 == 1), r.kt
    if nz % 8 == 1:
        assert r.kt[SINGLE40]["points"] == COLS, r.kt


def test_levels_per_wave_above_nz_is_nz():
    r = analysis(32, 9, "mixed", 1, "", 1000)
    assert r.info["levels_per_wave"] == 9
    assert np.array_equal(bits(r.out), bits(analysis(32, 9, "mixed", 0).out))


# ---- record path: waves that mix quadrature round classes ----------------------------------------
@pytest.mark.parametrize("k,nz", [(32, 9), (40, 2)])
def test_record_path_mixed_round_classes_columns_multiple_of_4(k, nz):
    """132 columns: the waves of option 0 and of the shared calls hold the same points, so the
    results are bit-equal although the waves mix the 15- and 23-node classes."""
    check(k, nz, "straddle", shares=(1, 2), levels=(0, 1, 3), nx=12)


@pytest.mark.parametrize("k,nz", [(32, 9), (40, 2)])
def test_record_path_mixed_round_classes_on_143_columns(k, nz):
    """143 columns: level kz starts at point 143 kz, so a column's wave-mates differ between
    option 0 and the shared calls, and a point of the 15-node class may run the 23-node rule
    under one and not the other.  Options 1 and 2 agree bit for bit at every split; against
    option 0 and the oracle the results meet INCR_TOL, with equal counters."""
    ref = analysis(k, nz, "straddle", 0)
    conditions("straddle", ref.cnt, k)
    got = [analysis(k, nz, "straddle", 1, "", lv) for lv in (0, 1, 3)]
    got.append(analysis(k, nz, "straddle", 2))
    for r in got:
        assert r.info["shared"] == 1 and r.cnt == ref.cnt
        assert np.array_equal(bits(r.out), bits(got[0].out))
    w = workload(k, nz, "straddle")
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    orc = w.var.copy()
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, w.alt, orc)), 16,
                                  C.byref(abi.Stats()))
    assert rc == 0
    differ = int(np.count_nonzero(bits(got[0].out) != bits(ref.out)))
    rel0 = increment_rel_rms(got[0].out, ref.out, w.var)
    rel_orc = increment_rel_rms(got[0].out, orc, w.var)
    print(f"k={k} nz={nz}: {differ} of {ref.out.size} words differ from option 0; "
          f"increment_rel_rms vs option 0 {rel0:.3e}, vs oracle {rel_orc:.3e}, "
          f"option 0 vs oracle {increment_rel_rms(ref.out, orc, w.var):.3e}")
    assert rel0 <= INCR_TOL and rel_orc <= INCR_TOL, (rel0, rel_orc)


@pytest.mark.parametrize("k,opts", [(64, ()), (80, (("big_batch", 64),))])
def test_one_point_per_wavefront_paths_are_exact_with_mixed_classes(k, opts):
    check(k, 9, "straddle", opts=opts, shares=(1,))


# ---- one-wavefront and hand-off paths ------------------------------------------------------------
@pytest.mark.parametrize("k,case,opts", [
    (16, "mixed", ()), (16, "trunc", ()), (50, "dense", ()), (50, "mixed", ()), (64, "dense", ()),
    (64, "trunc", ()), (64, "mixed", ()), (32, "mixed", (("split40", 0),)),
    (32, "dense", (("split40", 0),))])
def test_one_wavefront_path(k, case, opts):
    _, got = check(k, 9, case, opts=opts, shares=(1, 2) if k == 64 else (1,))
    for r in got:
        assert r.info["chunk_launches"] == 2 and r.info["levels_per_wave"] == 0, r.info
        group = [n for n in r.kt if n.startswith("solve_tq_multi_kernel<")]
        single = [n for n in r.kt if n.startswith("solve_tq_kernel<")]
        assert len(group) == 1 and group[0].endswith(", 8>"), r.kt
        assert r.kt[group[0]]["points"] == COLS * 8, r.kt
        assert len(single) == 1 and r.kt[single[0]]["points"] == COLS, r.kt


@pytest.mark.parametrize("nz", [2, 17])
def test_one_wavefront_path_other_chunks(nz):
    check(64, nz, "dense", shares=(1,))


@pytest.mark.parametrize("k,case", [(80, "mixed"), (80, "dense"), (128, "dense"), (128, "trunc"),
                                    (128, "mixed")])
def test_hand_off_path(k, case):
    """k = 80 runs KP = 96; big_batch = 64 splits the batch of 143 columns into three."""
    _, got = check(k, 9, case, opts=(("big_batch", 64),), shares=(1,))
    r, = got
    assert r.info["chunk_launches"] == 2, r.info
    heads = [n for n in r.kt if "_multi_kernel<" in n and not n.startswith("solve_tqb_tail")]
    tails = [n for n in r.kt if n.startswith("solve_tqb_tail_multi_kernel<")]
    assert len(heads) == 1 and len(tails) == 1, r.kt
    assert r.kt[heads[0]]["launches"] == r.kt[tails[0]]["launches"] == 3, r.kt
    assert r.kt[heads[0]]["points"] == r.kt[tails[0]]["points"] == COLS * 8, r.kt
    assert r.kt["solve_tqb_tail_kernel<%d, %d, %d>" % ((96, 32, 2) if k == 80 else (128, 64, 3))][
        "points"] == COLS, r.kt


def test_hand_off_path_option_2_and_two_levels():
    check(80, 2, "dense", opts=(("big_batch", 64),), shares=(2,))


# ---- geometry and plumbing at k = 32 --------------------------------------------------------------
@pytest.mark.parametrize("variant,case,opts", [
    ("staggered", "mixed", ()),
    ("pageable", "mixed", ()),
    ("pinned", "mixed", ()),
    ("", "mixed", (("max_batch", 256), ("info_window", 256))),
    ("", "mixed", (("split40_batch", 64),)),
    ("", "trunc", (("split40_batch", 64),)),
    ("", "mixed", (("index", 1),)),
    ("", "trunc", (("index", 1),)),
    ("rtpp", "dense", ()),
    ("rtps", "dense", ()),
    ("plain", "dense", ()),
    ("tune_q", "mixed", ()),
    ("tune_q", "dense", ()),
])
def test_plumbing(variant, case, opts):
    ref, got = check(32, 9, case, variant, opts)
    if variant == "staggered":  # the last column is not analysed
        for r in [ref] + got:
            assert np.array_equal(bits(r.out[..., -1]), bits(ref.var[..., -1]))
    if variant in ("rtpp", "rtps", "plain"):  # the flags matter
        assert not np.array_equal(bits(ref.out), bits(analysis(32, 9, case, 0).out))
    if variant == "tune_q":
        assert not np.array_equal(bits(ref.out), bits(analysis(32, 9, case, 0).out))
        assert "tune_q_kernel" in got[0].kt and got[0].kt["tune_q_kernel"]["points"] == COLS * 9
    if opts == (("split40_batch", 64),):
        assert got[0].kt[COLUMN]["launches"] == got[0].kt[ASSEMBLE]["launches"] == 3, got[0].kt


@pytest.mark.parametrize("k", [32, 64])
def test_host_slab_other_paths(k):
    check(k, 9, "dense", "pageable", shares=(2,) if k == 32 else (1,))


@pytest.mark.parametrize("k,opts", [(32, ()), (32, (("index", 1),)), (50, ())])
def test_several_batches_of_columns(k, opts):
    """29 x 23 = 667 columns in search batches of at most 256 with info windows of 256: three
    batches of columns, the search of one overlapping the solves of the one before, and the
    window boundaries among the columns."""
    o = (("max_batch", 256), ("info_window", 256)) + opts
    _, got = check(k, 3, "trunc", opts=o, nx=29, ny=23)
    assert got[0].kt[SEARCH]["launches"] == 3, got[0].kt


@pytest.mark.parametrize("k", [32, 64])
def test_gaspari_cohn(k):
    """weight_function = 1: the reference's fp32 Gaspari-Cohn weights give NaN analyses at some
    points; a point's NaN comes from its weights, so it holds at every level of the column."""
    ref, _ = check(k, 9, "dense", "gc")
    nan = np.isnan(ref.out).any(axis=0)  # (nz, ny, nx)
    print(f"gaspari-cohn k={k}: {int(nan[0].sum())} NaN columns of {COLS}")
    assert np.array_equal(nan, np.broadcast_to(nan[0], nan.shape))
    assert not np.array_equal(bits(ref.out), bits(analysis(k, 9, "dense", 0).out))


# ---- isolation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,share", [(32, 1), (32, 2), (64, 1), (80, 1)])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_a_bad_level_stays_in_its_level(k, share, bad):
    """One member of one level of one column is NaN or Inf: every other level of that column,
    and every other column, equals the clean run."""
    opts = (("big_batch", 64),) if k == 80 else ()
    clean = analysis(k, 9, "dense", share, "", 0, opts)
    dirty = analysis(k, 9, "dense", share, bad, 0, opts)
    same = analysis(k, 9, "dense", 0, bad, 0, opts)
    assert dirty.info["shared"] == 1
    assert dirty.cnt == same.cnt == clean.cnt
    assert np.array_equal(bits(dirty.out), bits(same.out))
    _, lev, j, i = BAD
    differs = (bits(dirty.out) != bits(clean.out)).any(axis=0)  # (nz, ny, nx)
    assert differs[lev, j, i]
    assert not np.isfinite(dirty.out[:, lev, j, i]).all()
    differs[lev, j, i] = False
    assert not differs.any(), np.argwhere(differs)


# ---- fall-backs -----------------------------------------------------------------------------------
def fallback(w, reason, opts=None, obs_set=None, vp=None, q1_mode=None):
    outs = []
    for share in (0, 1):
        o = dict(opts or {})
        o["column_share"] = share
        lib = Lib(w, o, obs_set=obs_set)
        try:
            out, cnt = lib.one(w.var, vp or w.vp)
            info = lib.c.column_info()
            outs.append((out, cnt))
            assert info.shared == 0 and info.columns == 0 and info.levels == 0
            assert info.reason == (reason if share else abi.COLUMN_REASON_OFF), info.as_dict()
        finally:
            lib.close()
    assert outs[0][1]["solved"] > 0
    assert outs[0][1] == outs[1][1]
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
    assert not np.array_equal(bits(outs[0][0]), bits(w.var))
    return outs[0][1]


def test_fallback_3d_type():
    fallback(workload(32, 9, "3d"), abi.COLUMN_REASON_3D)


def test_fallback_q1_undefined_family():
    """Two radar types under the replicating q1_mode: dbz has vclr <= 0 but the family's
    leftover vclr_inv is vr's 3-D one, the Q1 undefined case."""
    w = workload(32, 9, "dense")
    half = w.obs.shape[0] // 2
    ob = (abi.ObsSetBuilder()
          .add_radar(abi.RADAR_DBZ, w.obs_xyz[:half], w.obs[:half], w.hdxb[:, :half])
          .add_radar(abi.RADAR_VR, w.obs_xyz[half:], w.obs[half:], w.hdxb[:, half:]).build())
    vp = copy.deepcopy(w.vp)
    vp.radar[abi.RADAR_DBZ - 1] = abi.type_params(use_it=1, max_lz_pts=1000, hclr=6.0, vclr=-1.0,
                                                  err_muti=1.0, err_rej=8.0)
    vp.radar[abi.RADAR_VR - 1] = abi.type_params(use_it=1, max_lz_pts=1000, hclr=6.0, vclr=3.0,
                                                 err_muti=1.0, err_rej=8.0)
    cnt = fallback(w, abi.COLUMN_REASON_Q1, obs_set=ob, vp=vp)
    assert cnt["q1_undefined"] > 0


def test_fallback_one_level():
    fallback(workload(32, 1, "dense"), abi.COLUMN_REASON_NZ)


def test_fallback_jacobi_solver():
    fallback(workload(32, 9, "dense"), abi.COLUMN_REASON_PATH, {"solver": 1})


def test_fallback_one_kernel_big_path():
    fallback(workload(96, 9, "dense"), abi.COLUMN_REASON_PATH, {"big_path": 0})


def test_group_call_ignores_the_option():
    w = workload(32, 9, "dense")
    vars_ = [w.var, other_var(w, 101)]
    lib = Lib(w, {"column_share": 1})
    try:
        outs, cnt = lib.group(vars_, [w.vp] * 2)
        info = lib.c.column_info()
        assert info.shared == 0 and info.reason == abi.COLUMN_REASON_GROUP
        for out, var in zip(outs, vars_):
            one, cnt1 = lib.one(var, w.vp)  # shared
            assert lib.c.column_info().shared == 1
            assert cnt1 == cnt and np.array_equal(bits(one), bits(out))
    finally:
        lib.close()


# ---- the record cache -----------------------------------------------------------------------------
def test_cache_untouched():
    """A per-point call fills the record cache, a column-shared call with other type parameters
    follows, and the first call repeated still solves from the kept records."""
    w3, w2 = workload(32, 9, "3d"), workload(32, 9, "dense")
    lib = Lib(w3, {"column_share": 1}, reuse_default=True)
    try:
        first, cnt = lib.one(w3.var, w3.vp)
        assert lib.c.column_info().reason == abi.COLUMN_REASON_3D
        fill = lib.c.reuse_info()
        assert fill.batches_assembled > 0 and fill.batches_reused == 0 and fill.bytes_held > 0
        shared, _ = lib.one(w2.var, w2.vp)
        assert lib.c.column_info().shared == 1
        mid = lib.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == fill.bytes_held
        assert np.array_equal(bits(shared), bits(analysis(32, 9, "dense", 0).out))
        again, cnt2 = lib.one(w3.var, w3.vp)
        hit = lib.c.reuse_info()
        assert hit.batches_reused == fill.batches_assembled and hit.batches_assembled == 0
        assert cnt2 == cnt and np.array_equal(bits(again), bits(first))
    finally:
        lib.close()


# ---- against the truth, not only the twin ---------------------------------------------------------
@pytest.mark.parametrize("k,share", [(32, 1), (32, 2), (64, 1)])
def test_against_the_oracle(k, share):
    w = workload(k, 9, "dense")
    r = analysis(k, 9, "dense", share)
    assert r.info["shared"] == 1
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
    print(f"k={k} option {share}: increment_rel_rms vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= INCR_TOL, rel


# ---- argument errors ------------------------------------------------------------------------------
def test_argument_errors():
    c = abi.Core(32, device=0)
    try:
        for name, value in (("column_share", -1), ("column_share", 3), ("column_levels", -1)):
            with pytest.raises(abi.CwblError, match="CWBL_ERR_ARG"):
                c.set_option(name, value)
        c.set_option("column_share", 2)
        c.set_option("column_levels", 5)
    finally:
        c.finalize()


def test_init_resets_the_options():
    w = workload(32, 9, "dense")
    lib = Lib(w, {"column_share": 1, "column_levels": 3})
    lib.close()
    lib = Lib(w)
    try:
        lib.one(w.var, w.vp)
        info = lib.c.column_info()
        assert info.shared == 0 and info.reason == abi.COLUMN_REASON_OFF
    finally:
        lib.close()
