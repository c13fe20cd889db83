"""GPU tests of CWBL_OPT_COLUMN_REUSE: the column cache.  A call that is shared per column
(CWBL_OPT_COLUMN_SHARE) keeps each column's assembled record (k = 17..40) or factor
(k = 41..64, k = 65..96) within a budget, and the next shared call of the same localisation on
the same x and y solves all its levels from them, whatever its nz, alt and epilogue flags:
MU (nz = 1), P (nz) and PH (nz + 1) pay one search, assembly and reduction.

The yardstick of every comparison is the same call on a fresh core with column_reuse = 0, never
an earlier call of the core under test: np.array_equal on the bit patterns of the whole slab and
equal counters.

Workload: test_gpu_column_share.py's, 13 x 11 = 143 columns with the obs set of the nz = 10
workload; a call analyses the levels [0, nz) of its var with an alt array of its own.  12 x 11
for the staggered case, 29 x 23 = 667 columns in three batches for the budget cases, big_batch =
64 for three sub-batches on the hand-off path.  k = 97..128 is not served by the option: it is
among the ignored classes.
"""
import collections
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

from cwbl import abi
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, counters, other_var, to_dev
from test_gpu_column_factor import BIG, fill_kernel, kp_of, level_kernel
from test_gpu_column_share import ASSEMBLE, BAD, COLS, COLUMN, INCR_TOL, NX, NY, SEARCH, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NZMAX = 10                    # the obs set and var of every call: the nz = 10 workload's
SEQ = (1, 9, 10)              # MU, P, PH
KS = (32, 41, 50, 64, 65, 80, 96)
KS3 = (32, 50, 80)            # one k per path
BUDGET = 64                   # MiB: every column of the small workloads fits
FORM = {40: abi.COLUMN_FORM_RECORDS, 48: abi.COLUMN_FORM_WAVE, 56: abi.COLUMN_FORM_WAVE,
        64: abi.COLUMN_FORM_WAVE, 96: abi.COLUMN_FORM_BIG}
# bytes per cached column: AsmRecord<40>, WaveFactor<KP> (KP (KP - 1) / 2 + 5 KP words),
# BigFactor<96, 32> (4977 words)
COLUMN_BYTES = {40: 6880, 48: 10944, 56: 14560, 64: 18688, 96: 39816}

Res = collections.namedtuple("Res", "out cnt info reuse kt prep")


def kpc(k):
    return 40 if k <= 40 else kp_of(k)


def all_kernel(k):
    """What solves every level of a cached column on a hit."""
    kp = kpc(k)
    return (COLUMN if kp == 40 else "solve_tqb_factor_column_all_kernel<96, 32>" if kp == 96
            else f"solve_tq_wave_factor_column_all_kernel<{kp}>")


def base_opts(k, more=()):
    """column_share = 1 with column_factor = 1 above k = 40 (and three sub-batches above 64)."""
    o = (("column_share", 1),)
    if k > 40:
        o += (("column_factor", 1),)
    if k > 64:
        o += BIG
    return o + tuple(more)


def vp_of(w, variant):
    vp = copy.deepcopy(w.vp)
    tp = vp.radar[w.radar_type - 1]
    if variant == "rtpp":
        vp.use_rtps = 0
    elif variant == "rtps":
        vp.use_rtpp = 0
    elif variant == "plain":
        vp.use_rtpp = vp.use_rtps = 0
    elif variant == "alphas":
        vp.rtpp_alpha, vp.rtps_alpha = 0.35, 0.65
    elif variant == "tune_q":
        vp.tune_q = 1
    elif variant == "hclr":
        tp.hclr = tp.hclr * 0.75
    elif variant == "infl":
        vp.multi_infl = 1.3
    elif variant == "3d":
        tp.vclr = 3.0
    return vp


def var_of(w, variant, nz):
    var = w.var
    if variant in ("nan", "inf"):
        var = var.copy()
        var[BAD] = np.nan if variant == "nan" else np.inf
    return np.ascontiguousarray(var[:, :nz])


class Seq:
    """One core on the nz = 10 workload's obs set, x and y; every call brings the levels [0, nz)
    of var and an alt array of its own (shifted per nz: alt is not part of the key)."""

    def __init__(self, k, case, opts, nx=NX, ny=NY, host=False, wf=0, record_reuse=False):
        self.w = workload(k, NZMAX, case, nx, ny)
        self.lib = Lib(self.w, dict(opts), host=host, weight_function=wf,
                       reuse_default=record_reuse)
        self.keep, self.pending = [], []

    def same(self, r, *args, **kw):
        """r against yard(*args, **kw), compared by close(): the library's state is one per
        process, so the yardstick's core cannot live beside this one."""
        self.pending.append((r, args, kw))
        return r

    def call(self, nz, variant="", pinned=False):
        w, lib = self.w, self.lib
        var, vp = var_of(w, variant, nz), vp_of(w, variant)
        ix_lim = w.nx - 1 if variant == "staggered" else None
        alt = w.alt[:nz] + np.float32(7.0 * nz)
        if ix_lim:
            alt = alt[:, :, :ix_lim]
        alt = np.ascontiguousarray(alt, np.float32)
        alt = alt if lib.host else to_dev(alt)
        if pinned:
            hold = torch.empty(var.shape, dtype=torch.float32).pin_memory()
            self.keep.append(hold)
            buf = hold.numpy()
            buf[...] = var
        else:
            buf, = lib.buffers([var])
        lib.c.set_kernel_timing(True)  # (clears the sums: the table is this call's)
        st = lib.c.analyze_var(vp, lib.slab(buf, ix_lim, alt=alt))
        out = np.array(lib.fetch(buf), copy=True)
        return Res(out, counters(st), lib.c.column_info().as_dict(),
                   lib.c.column_reuse_info().as_dict(), lib.c.kernel_times(),
                   lib.c.prep_info().as_dict())

    def close(self, compare=True):
        self.lib.close()
        pending, self.pending = self.pending, []
        for r, args, kw in pending if compare else ():
            same(r, yard(*args, **kw))


@functools.lru_cache(maxsize=None)
def yard(k, case, nz, variant="", opts=None, nx=NX, ny=NY, host=False, wf=0, xshift=False):
    """The yardstick: the call alone on a fresh core with column_reuse = 0.  Computed once per
    argument set, shared and left unchanged."""
    o = dict(base_opts(k) if opts is None else opts)
    o["column_reuse"] = 0
    s = Seq(k, case, o, nx, ny, host, wf)
    try:
        if xshift:
            shift_x(s)
        r = s.call(nz, variant)
        assert r.reuse["columns_reused"] == r.reuse["columns_filled"] == 0, r.reuse
        assert r.reuse["bytes_held"] == 0 and r.reuse["form"] == abi.COLUMN_FORM_NONE, r.reuse
        assert not [n for n in r.kt if "_column_all_kernel" in n], r.kt
        return r
    finally:
        s.close()


def shift_x(s):
    """x rewritten in place behind the same pointer: one coordinate moved by a metre."""
    s.lib.x[3, 4] += 1.0
    if not s.lib.host:
        torch.cuda.synchronize()


def same(r, ref):
    assert r.cnt == ref.cnt, (r.cnt, ref.cnt)
    assert np.array_equal(bits(r.out), bits(ref.out))


def is_fill(r, k, nz, cols=COLS):
    """r searched and assembled per column, and left every column in the cache."""
    assert r.info["shared"] == 1 and r.info["levels"] == nz and r.info["columns"] == cols, r.info
    assert r.reuse["columns_filled"] == cols and r.reuse["columns_reused"] == 0, r.reuse
    assert r.reuse["batches_reused"] == 0 and r.reuse["form"] == FORM[kpc(k)], r.reuse
    assert r.reuse["bytes_held"] >= cols * COLUMN_BYTES[kpc(k)], r.reuse
    assert r.kt[SEARCH]["points"] == cols, r.kt
    if k <= 40:
        assert r.kt[ASSEMBLE]["points"] == cols and r.kt[COLUMN]["points"] == cols * nz, r.kt
    else:
        assert r.kt[fill_kernel(k)]["points"] == cols, r.kt
        assert all_kernel(k) not in r.kt, r.kt
        if nz > 1:
            assert r.kt[level_kernel(k)]["points"] == cols * (nz - 1), r.kt
        assert r.info["from_factor"] == 1, r.info
    assert not [n for n in r.kt if "_multi_kernel<" in n], r.kt


def is_hit(r, k, nz, cols=COLS):
    """r solved every level of every column from the cache, in launches of the all-levels kernel
    alone (tune_q aside)."""
    assert r.info["shared"] == 1 and r.info["levels"] == nz and r.info["columns"] == cols, r.info
    assert r.reuse["columns_reused"] == cols and r.reuse["columns_filled"] == 0, r.reuse
    assert r.reuse["batches_reused"] >= 1 and r.reuse["form"] == FORM[kpc(k)], r.reuse
    assert r.reuse["ms_compare"] > 0.0, r.reuse
    assert sorted(n for n in r.kt if n != "tune_q_kernel") == [all_kernel(k)], r.kt
    assert r.kt[all_kernel(k)]["points"] == cols * nz, r.kt
    # no obs preparation, tree or bin work either
    assert r.prep["trees_built"] == r.prep["bins_built"] == 0, r.prep
    assert r.prep["ms_columns"] == 0.0 and r.prep["ms_bins"] == 0.0, r.prep


def reuse_opts(k, more=(), budget=BUDGET):
    return base_opts(k, (("column_reuse", budget),) + tuple(more))


# ---- 1. MU -> P -> PH on one core ------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "mixed", "trunc"])
@pytest.mark.parametrize("k", KS)
def test_sequence(k, case):
    """nz = 1 fills, nz = 9 and nz = 10 hit; every slab is the yardstick's."""
    s = Seq(k, case, reuse_opts(k))
    try:
        got = [s.call(nz) for nz in SEQ]
    finally:
        s.close()
    is_fill(got[0], k, 1)
    for r, nz in zip(got[1:], SEQ[1:]):
        is_hit(r, k, nz)
        assert r.kt[all_kernel(k)]["launches"] == (3 if k > 64 else 1), r.kt
        assert r.reuse["bytes_held"] == got[0].reuse["bytes_held"]
    for r, nz in zip(got, SEQ):
        same(r, yard(k, case, nz))
    ref = yard(k, case, 9)
    assert not np.array_equal(bits(ref.out), bits(var_of(s.w, "", 9)))  # something was analysed
    if case == "trunc":
        assert ref.cnt["lz_truncated"] > 0
    if case == "mixed":
        assert 0 < ref.cnt["solved"] < ref.cnt["points"]
    # the call of one level: shared only with the option on, and bit for bit the per-point call
    assert got[0].info["levels_per_wave"] == (1 if k <= 40 else 0), got[0].info
    off = yard(k, case, 1)
    assert off.info["shared"] == 0 and off.info["reason"] == abi.COLUMN_REASON_NZ, off.info
    point = yard(k, case, 1, "", (("column_share", 0),))
    assert point.info["reason"] == abi.COLUMN_REASON_OFF
    same(got[0], point)


@pytest.mark.parametrize("k", KS3)
def test_sequence_filled_by_the_deepest_call(k):
    """Any eligible call fills: nz = 10 first, then nz = 1 and nz = 9 hit; option 2 of
    column_share caches the same one-factor form."""
    o = dict(reuse_opts(k), column_share=2)
    s = Seq(k, "dense", o)
    try:
        got = [s.call(nz) for nz in (10, 1, 9)]
    finally:
        s.close()
    is_fill(got[0], k, 10)
    is_hit(got[1], k, 1)
    is_hit(got[2], k, 9)
    for r, nz in zip(got, (10, 1, 9)):
        same(r, yard(k, "dense", nz))


# ---- 2. what may change on a hit --------------------------------------------------------------
@pytest.mark.parametrize("k", KS3)
def test_flags_and_level_splits_still_hit(k):
    s = Seq(k, "dense", reuse_opts(k))
    try:
        is_fill(s.call(9), k, 9)
        for variant in ("rtpp", "rtps", "plain", "alphas", "tune_q"):
            r = s.same(s.call(9, variant), k, "dense", 9, variant)
            is_hit(r, k, 9)
            if variant == "tune_q":
                assert r.kt["tune_q_kernel"]["points"] == COLS * 9, r.kt
        for lv in (1, 3, 9):  # forced level splits: the option voids nothing
            s.lib.c.set_option("column_levels", lv)
            r = s.same(s.call(9), k, "dense", 9)
            is_hit(r, k, 9)
            assert r.info["levels_per_wave"] == lv, r.info
    finally:
        s.close()
    assert not np.array_equal(bits(yard(k, "dense", 9, "plain").out),
                              bits(yard(k, "dense", 9).out))  # the flags matter


@pytest.mark.parametrize("k", KS3)
@pytest.mark.parametrize("pipe", [0, 1])
def test_host_slabs_still_hit(k, pipe):
    """Pageable and page-locked host slabs, whole or piped per column batch."""
    s = Seq(k, "mixed", reuse_opts(k, (("host_pipe", pipe),)), host=True)
    try:
        is_fill(s.call(1), k, 1)
        for pinned in (False, True):
            is_hit(s.same(s.call(9, pinned=pinned), k, "mixed", 9), k, 9)
    finally:
        s.close()


# ---- 3. misses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS3)
def test_misses_refill(k):
    s = Seq(k, "dense", reuse_opts(k))
    try:
        is_fill(s.call(1), k, 1)
        is_hit(s.call(9), k, 9)
        # another hclr, another multi_infl: other keys
        for variant in ("hclr", "infl"):
            is_fill(s.same(s.call(9, variant), k, "dense", 9, variant), k, 9)
            is_hit(s.same(s.call(10, variant), k, "dense", 10, variant), k, 10)
        # the obs set again
        is_fill(s.call(9), k, 9)
        s.lib.c.set_obs(abi.ObsSetBuilder().add_radar(s.w.radar_type, s.w.obs_xyz, s.w.obs,
                                                      s.w.hdxb).build())
        is_fill(s.same(s.call(9), k, "dense", 9), k, 9)
        # an option
        is_hit(s.call(10), k, 10)
        s.lib.c.set_option("info_window", 512)
        is_fill(s.same(s.call(10), k, "dense", 10), k, 10)
        # ix_lim: the staggered slab, 12 x 11 columns
        cols = (NX - 1) * NY
        r = s.same(s.call(9, "staggered"), k, "dense", 9, "staggered")
        is_fill(r, k, 9, cols)
        is_hit(s.same(s.call(10, "staggered"), k, "dense", 10, "staggered"), k, 10, cols)
        assert np.array_equal(bits(r.out[..., -1]), bits(var_of(s.w, "", 9)[..., -1]))
        # x rewritten in place behind an equal key
        is_fill(s.call(9), k, 9)
        shift_x(s)
        r = s.same(s.call(9), k, "dense", 9, xshift=True)
        is_fill(r, k, 9)
        assert r.reuse["ms_compare"] > 0.0
        is_hit(s.same(s.call(1), k, "dense", 1, xshift=True), k, 1)
    finally:
        s.close()


@pytest.mark.parametrize("k", KS3)
def test_a_3d_call_in_between_leaves_the_cache(k):
    s = Seq(k, "dense", reuse_opts(k))
    try:
        is_fill(s.call(1), k, 1)
        held = s.call(9).reuse["bytes_held"]
        r = s.call(9, "3d")
        assert r.info["shared"] == 0 and r.info["reason"] == abi.COLUMN_REASON_3D, r.info
        assert r.reuse["columns_reused"] == r.reuse["columns_filled"] == 0, r.reuse
        assert r.reuse["bytes_held"] == held
        s.same(r, k, "dense", 9, "3d")
        is_hit(s.same(s.call(10), k, "dense", 10), k, 10)
    finally:
        s.close()


# ---- 4. and 5. budgets ----------------------------------------------------------------------------
def three_batches(k, budget):
    return reuse_opts(k, (("max_batch", 256), ("info_window", 256)), budget)


@pytest.mark.parametrize("k", KS3)
def test_partial_budget(k):
    """29 x 23 = 667 columns in batches of 256, 256 and 155 (max_batch = 256, whole list groups
    of 64): a budget that holds the first batch's 256 + 1 entries and not the second's."""
    per = COLUMN_BYTES[kpc(k)]
    budget = math.ceil(257 * per / 2 ** 20)
    assert 257 * per <= budget * 2 ** 20 < 2 * 257 * per
    o = three_batches(k, budget)
    base = tuple((n, v) for n, v in o if n != "column_reuse")
    s = Seq(k, "trunc", o, 29, 23)
    try:
        a, b = s.call(1), s.call(3)
    finally:
        s.close()
    assert a.reuse["columns_filled"] == 256 and a.reuse["batches_reused"] == 0, a.reuse
    assert a.kt[SEARCH]["launches"] == 3, a.kt
    assert b.reuse["columns_reused"] == 256 and b.reuse["batches_reused"] == 1, b.reuse
    assert b.kt[all_kernel(k)]["points"] >= 256 * 3, b.kt
    assert b.kt[SEARCH]["launches"] == 2 and b.kt[SEARCH]["points"] == 667 - 256, b.kt
    if k <= 40:
        assert b.kt[ASSEMBLE]["points"] == 667 - 256 and b.kt[COLUMN]["points"] == 667 * 3, b.kt
    else:
        assert b.kt[fill_kernel(k)]["points"] == 667 - 256, b.kt
        assert b.kt[level_kernel(k)]["points"] == (667 - 256) * 2, b.kt
    same(a, yard(k, "trunc", 1, "", base, 29, 23))
    same(b, yard(k, "trunc", 3, "", base, 29, 23))


@pytest.mark.parametrize("k", KS3)
def test_every_batch_cached(k):
    """The same three batches within the budget: three cached batches, the info windows among
    them."""
    o = three_batches(k, BUDGET)
    base = tuple((n, v) for n, v in o if n != "column_reuse")
    s = Seq(k, "trunc", o, 29, 23)
    try:
        a, b = s.call(3), s.call(1)
    finally:
        s.close()
    is_fill(a, k, 3, 667)
    is_hit(b, k, 1, 667)
    assert b.reuse["batches_reused"] == 3
    same(a, yard(k, "trunc", 3, "", base, 29, 23))
    same(b, yard(k, "trunc", 1, "", base, 29, 23))


@pytest.mark.parametrize("k", KS3)
def test_no_budget_runs_as_without_the_option(k):
    """A budget below one batch's need, and column_reuse = 0 after a fill: nothing is held and
    the calls run what they run today."""
    per = COLUMN_BYTES[kpc(k)]
    o = three_batches(k, 1)
    assert 257 * per > 2 ** 20
    base = tuple((n, v) for n, v in o if n != "column_reuse")
    ref = yard(k, "trunc", 3, "", base, 29, 23)
    s = Seq(k, "trunc", o, 29, 23)
    try:
        for _ in range(2):
            r = s.call(3)
            assert r.reuse["bytes_held"] == 0 and r.reuse["form"] == abi.COLUMN_FORM_NONE, r.reuse
            assert r.reuse["columns_filled"] == r.reuse["columns_reused"] == 0, r.reuse
            same(r, ref)
            assert {n: t["points"] for n, t in r.kt.items()} == \
                   {n: t["points"] for n, t in ref.kt.items()}
        s.lib.c.set_option("column_reuse", BUDGET)
        is_fill(s.call(3), k, 3, 667)
        s.lib.c.set_option("column_reuse", 0)
        r = s.call(3)
        assert r.reuse["bytes_held"] == 0 and r.reuse["columns_reused"] == 0, r.reuse
        same(r, ref)
        assert sorted(r.kt) == sorted(ref.kt), (r.kt, ref.kt)
        r = s.call(1)  # and a call of one level is per point again
        assert r.info["shared"] == 0 and r.info["reason"] == abi.COLUMN_REASON_NZ, r.info
    finally:
        s.close()


# ---- 6. the record cache ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,option", [(32, None), (50, "wave_reuse"), (80, "big_reuse")])
def test_record_cache_left_as_it_was(k, option):
    """A per-point call (a 3-D type) fills the record cache; a column sequence follows; the
    per-point call repeated still hits, and the column cache still serves."""
    o = dict(reuse_opts(k))
    if option:
        o[option] = 1
    s = Seq(k, "dense", o, record_reuse=True)
    try:
        first = s.same(s.call(9, "3d"), k, "dense", 9, "3d")
        fill = s.lib.c.reuse_info()
        assert fill.batches_assembled > 0 and fill.batches_reused == 0 and fill.bytes_held > 0
        is_fill(s.call(1), k, 1)
        is_hit(s.call(9), k, 9)
        mid = s.lib.c.reuse_info()
        assert mid.batches_reused == 0 and mid.bytes_held == fill.bytes_held
        again = s.call(9, "3d")
        hit = s.lib.c.reuse_info()
        assert hit.batches_reused == fill.batches_assembled and hit.batches_assembled == 0
        assert again.reuse["columns_reused"] == 0
        same(again, first)
        is_hit(s.call(10), k, 10)
    finally:
        s.close()


# ---- 7. special values --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS3)
def test_gaspari_cohn_on_a_hit(k):
    """weight_function = 1: NaN analyses at some columns, at every level of them."""
    s = Seq(k, "dense", reuse_opts(k), wf=1)
    try:
        is_fill(s.call(1), k, 1)
        r = s.call(9)
    finally:
        s.close()
    is_hit(r, k, 9)
    same(r, yard(k, "dense", 9, wf=1))
    nan = np.isnan(r.out).any(axis=0)  # (nz, ny, nx)
    print(f"gaspari-cohn k={k}: {int(nan[0].sum())} NaN columns of {COLS}")
    assert np.array_equal(nan, np.broadcast_to(nan[0], nan.shape))


@pytest.mark.parametrize("k", KS3)
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_a_bad_level_stays_in_its_level_on_a_hit(k, bad):
    s = Seq(k, "dense", reuse_opts(k))
    try:
        is_fill(s.call(1), k, 1)
        clean, dirty = s.call(9), s.call(9, bad)
    finally:
        s.close()
    is_hit(dirty, k, 9)
    same(dirty, yard(k, "dense", 9, bad))
    assert dirty.cnt == clean.cnt
    _, lev, j, i = BAD
    differs = (bits(dirty.out) != bits(clean.out)).any(axis=0)  # (nz, ny, nx)
    assert differs[lev, j, i]
    assert not np.isfinite(dirty.out[:, lev, j, i]).all()
    differs[lev, j, i] = False
    assert not differs.any(), np.argwhere(differs)


# ---- 8. where the option is accepted and ignored -------------------------------------------------------
@pytest.mark.parametrize("k,more", [(16, ()), (32, (("split40", 0),)), (50, (("solver", 1),)),
                                    (80, (("big_path", 0),)), (112, BIG), (128, BIG)])
def test_ignored_classes(k, more):
    more = (("column_share", 1), ("column_factor", 1)) + tuple(more)
    on = more + (("column_reuse", BUDGET),)
    s = Seq(k, "dense", on)
    try:
        got = [s.call(nz) for nz in (9, 9, 1)]
    finally:
        s.close()
    for r, nz in zip(got, (9, 9, 1)):
        ref = yard(k, "dense", nz, "", more)
        same(r, ref)
        assert r.info == ref.info, (r.info, ref.info)
        assert r.reuse == ref.reuse, r.reuse
        assert {n: t["points"] for n, t in r.kt.items()} == \
               {n: t["points"] for n, t in ref.kt.items()}
    assert got[2].info["reason"] == abi.COLUMN_REASON_NZ


def test_group_calls_ignore_the_option():
    k = 32
    w = workload(k, NZMAX, "dense")
    vars_ = [w.var, other_var(w, 7)]
    outs = []
    for budget in (0, BUDGET):
        lib = Lib(w, dict(base_opts(k), column_reuse=budget))
        try:
            outs.append(lib.group(vars_, [w.vp] * 2))
            info, reuse = lib.c.column_info(), lib.c.column_reuse_info()
            assert info.shared == 0 and info.reason == abi.COLUMN_REASON_GROUP
            assert reuse.columns_filled == reuse.columns_reused == reuse.bytes_held == 0
        finally:
            lib.close()
    (a, ca), (b, cb) = outs
    assert ca == cb and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_argument_errors_and_init():
    c = abi.Core(50, device=0)
    try:
        for value in (-1, (1 << 24) + 1):
            with pytest.raises(abi.CwblError, match="CWBL_ERR_ARG"):
                c.set_option("column_reuse", value)
        c.set_option("column_reuse", 8)
        c.set_option("column_reuse", 0)
        assert c.column_reuse_info().bytes_held == 0
    finally:
        c.finalize()
    # cwbl_init resets the option: a call of one level is per point again
    s = Seq(50, "dense", reuse_opts(50))
    s.close()
    s = Seq(50, "dense", base_opts(50))
    try:
        r = s.call(1)
        assert r.info["shared"] == 0 and r.reuse["columns_filled"] == 0, (r.info, r.reuse)
    finally:
        s.close()


# ---- 9. against the truth, not only the twin -------------------------------------------------------------
@pytest.mark.parametrize("k", KS3)
def test_a_hit_against_the_oracle(k):
    s = Seq(k, "dense", reuse_opts(k))
    try:
        is_fill(s.call(1), k, 1)
        r = s.call(9)
    finally:
        s.close()
    is_hit(r, k, 9)
    w = s.w
    var = var_of(w, "", 9)
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    ref = var.copy()
    ost = abi.Stats()
    alt = np.ascontiguousarray(w.alt[:9] + np.float32(63.0))
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, alt, ref)), 16, C.byref(ost))
    assert rc == 0
    assert r.cnt["solved"] == ost.solved and r.cnt["nobs_sum"] == ost.nobs_sum
    assert r.cnt["max_p"] == ost.max_p
    rel = increment_rel_rms(r.out, ref, var)
    moved = np.count_nonzero(bits(ref) != bits(var))
    print(f"k={k}: increment_rel_rms of a hit vs oracle {rel:.3e} ({moved} analysed values)")
    assert moved > 0
    assert rel <= INCR_TOL, rel
