"""GPU tests of multi-variable GTS obs types (SOUND, SYNOP, GPSPW, METAR, and a type of three
variables) above k = 40, where the golden driver cases stop: the one-wavefront path at
k = 41..64, the hand-off path at k = 65..128 and its one-kernel form, their group forms, the
three factor caches, column sharing, the device-built index and a device-resident obs set.
With nvar > 1 the stagers of cwbl_device.h (stage_columns, stage_columns_pair,
stage_columns_pipe) divide the (obs, variable) pair index by nvar, chunks of 32 or 64 pairs cut
through observations, 2-D and 3-D trees meet in one call with both Q1 rules, and obs_prep_kernel
applies is_assim, any(qc >= 0), error * err_muti[v] and err_rej[v] at kp = 48 .. 128 with
k < kp padding.  None of that happens with a radar type.

Workload: tests/gts_cases.py (720 points, batches of 256, 256 and 208); its conditions are
asserted on the oracle alone in tests/test_gts_cases.py.  The yardsticks: the oracle at
INCR_TOL (the project's path-versus-oracle bar) with NaNs at identical positions and equal
counters for the plain calls; np.array_equal on the bit patterns (NaN-aware) and equal counters
for every comparison of two of the library's own paths that evaluate the same expressions;
1e-9 (the bar of test_gpu_index) where only the column order changes.
"""
import copy
import functools

import numpy as np
import pytest

import gts_cases as gc
from cwbl import abi
from factor_cache_suite import BIG, ROWS, WAVE
from helpers import increment_rel_rms
from reuse_harness import BATCH, Run, is_hit, is_miss, same
from test_gpu_analyze_vars import Lib, bits, to_dev, variables
from test_gpu_analyze_vars_big_mixed import nan_aware_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INCR_TOL = 1e-6
OPTS = {"max_batch": 256, "record_reuse": 0}
ORACLE_COUNTERS = ("solved", "nobs_sum", "lz_truncated", "max_p", "q1_undefined", "ntrees")
BASE_KS = (41, 50, 56, 64, 65, 80, 96, 97, 112, 128)  # every KP above 40: k = KP, most padded
SINGLE = [("base", k) for k in BASE_KS] + [(v, k) for v in gc.VARIANTS[1:] for k in (64, 96, 128)]


def kernels_of(k, big_path=1):
    """The solve kernels of a cwbl_analyze_var call at k."""
    if k <= 40:
        return ("solve_tq40_kernel<40, 0>",)
    if k <= 64:
        return (f"solve_tq_kernel<{(k + 7) // 8 * 8}, false>",)
    if not big_path:
        return (f"solve_tq_big_kernel<{96 if k <= 96 else 128}, false>",)
    if k <= 96:
        return ("solve_tq_big_kernel<96, false, 32>", "solve_tqb_tail_kernel<96, 32, 2>")
    return ("solve_tq_rows_kernel<128, 64>", "solve_tqb_tail_kernel<128, 64, 3>")


def group_kernels_of(k):
    """What the names of a three-variable cwbl_analyze_vars call's solve kernels start with."""
    if k <= 64:
        return (f"solve_tq_multi_kernel<{(k + 7) // 8 * 8}, ",)
    if k <= 96:
        return ("solve_tq_big_multi_kernel<96, 32, ", "solve_tqb_tail_multi_kernel<96, 32, ")
    return ("solve_tq_rows_multi_kernel<128, 64, ", "solve_tqb_tail_multi_kernel<128, 64, ")


class GtsLib(Lib):
    """Lib on a gts_cases.Case: the case's obs set (host arrays, or memory = MEM_DEVICE),
    weight function and Q1 mode; batches of 256 and no record cache unless `opts` says so."""

    def __init__(self, case, opts=None, memory=abi.MEM_HOST):
        self.w, self.host = case, False
        self.c = abi.Core(case.k, device=0, weight_function=case.weight_function,
                          norain_value=gc.NORAIN, q1_mode=case.q1_mode,
                          options=dict(OPTS, **(opts or {})))
        dev = (lambda a: torch.from_numpy(a).to("cuda:0")) if memory == abi.MEM_DEVICE else None
        self.c.set_obs(case.obs_set(memory, dev))
        self.x, self.y, self.alt = (to_dev(a) for a in (case.x, case.y, case.alt))


def analyse(case, var=None, opts=None, memory=abi.MEM_HOST):
    """One cwbl_analyze_var on a fresh core: (analysis, counters, kernel times, column_info)."""
    lib = GtsLib(case, opts, memory)
    try:
        lib.c.set_kernel_timing(True)
        out, cnt = lib.one(case.var if var is None else var, case.vp)
        return out, cnt, lib.c.kernel_times(), lib.c.column_info().as_dict()
    finally:
        lib.close()


@functools.lru_cache(maxsize=None)
def plain(variant, k):
    """The plain call of a case (max_batch = 256, every option at its default but the record
    cache, which is off); shared, never modified."""
    return analyse(gc.make(variant, k))


def against_oracle(case, out, cnt, ref, ost, var=None):
    """The single call's checks against the oracle's analysis and counters."""
    var = case.var if var is None else var
    for name in ORACLE_COUNTERS:
        assert cnt[name] == getattr(ost, name), (name, cnt, getattr(ost, name))
    assert cnt["points"] == case.points and cnt["nonconverged"] == 0, cnt
    rel = increment_rel_rms(out, ref, var)
    print(f"{case.variant} k={case.k}: vs oracle {rel:.3e}; {cnt}; "
          f"{int(np.isnan(out).any(axis=0).sum())} NaN points")
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    assert rel <= INCR_TOL, rel
    untouched = np.all(bits(ref) == bits(var), axis=0)
    assert untouched.sum() == case.points - ost.solved
    assert np.array_equal(bits(out[:, untouched]), bits(var[:, untouched]))


# ---- single calls against the oracle -----------------------------------------------------------
@pytest.mark.parametrize("variant,k", SINGLE, ids=[f"{v}-{k}" for v, k in SINGLE])
def test_single_call_vs_oracle(variant, k):
    case = gc.make(variant, k)
    ref, ost = gc.oracle_ref(variant, k)
    out, cnt, kt, _ = plain(variant, k)
    against_oracle(case, out, cnt, ref, ost)
    for name in kernels_of(k):
        assert name in kt and kt[name]["points"] == case.points, (name, kt)


@pytest.mark.parametrize("k", [33, 40])
def test_record_path_vs_oracle(k):
    """The generator pinned where the golden driver cases already agree: a failure above 40 is
    then not the workload's."""
    case = gc.make("base", k)
    out, cnt, kt, _ = plain("base", k)
    against_oracle(case, out, cnt, *gc.oracle_ref("base", k))
    assert kernels_of(k)[0] in kt and "assemble_record_kernel<4>" in kt, kt


@pytest.mark.parametrize("k", [96, 128])
def test_one_kernel_big_path_vs_oracle(k):
    """big_path = 0: stage_columns with 256 threads, the third stager."""
    case = gc.make("base", k)
    out, cnt, kt, _ = analyse(case, opts={"big_path": 0})
    against_oracle(case, out, cnt, *gc.oracle_ref("base", k))
    name, = kernels_of(k, big_path=0)
    assert name in kt and kt[name]["points"] == case.points, kt
    assert not [n for n in kt if n.startswith(("solve_tqb_tail", "solve_tq_rows"))], kt


# ---- group calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["base", "truncated", "gaspari_cohn"])
@pytest.mark.parametrize("k", [64, 96, 128])
def test_group_equals_single_calls(k, variant):
    case = gc.make(variant, k)
    vars_ = variables(case, 3)
    lib = GtsLib(case)
    try:
        singles = [lib.one(v, case.vp) for v in vars_]
        lib.c.set_kernel_timing(True)
        outs, cnt = lib.group(vars_, [case.vp] * 3)
        kt = lib.c.kernel_times()
    finally:
        lib.close()
    for start in group_kernels_of(k):
        assert len([n for n in kt if n.startswith(start)]) == 1, (start, kt)
    assert not [n for n in kt if n in kernels_of(k)], kt
    assert cnt["solved"] > 0 and cnt["nonconverged"] == 0
    for i, (out, (one, scnt)) in enumerate(zip(outs, singles)):
        assert cnt == scnt, (i, cnt, scnt)
        assert nan_aware_equal(out, one), i
    assert nan_aware_equal(singles[0][0], plain(variant, k)[0])  # (what the oracle checked)
    for i in range(3):
        for j in range(i + 1, 3):
            assert not nan_aware_equal(outs[i], outs[j]), (i, j)


# ---- factor caches -----------------------------------------------------------------------------
class GtsInputs:
    """What reuse_harness.Run reads of its Inputs, for a gts_cases.Case."""

    def __init__(self, case):
        self.case, self.k = case, case.k
        self.x, self.y, self.alt = case.x.copy(), case.y.copy(), case.alt.copy()
        self.vp = copy.deepcopy(case.vp)
        self.ix_lim = None
        self.options = {}


class GtsRun(Run):
    """reuse_harness.Run with the case's obs set."""

    def sync(self, inp):
        self.inp = inp
        for dst, src in ((self.x, inp.x), (self.y, inp.y), (self.alt, inp.alt)):
            dst.copy_(torch.from_numpy(src))
        if inp.case is not self.hdxb:
            self.c.set_obs(inp.case.obs_set())
            self.hdxb = inp.case


CACHES = [(form, k) for form, ks in ((WAVE, (64, 50)), (BIG, (96, 65)), (ROWS, (128, 97)))
          for k in ks]


@pytest.mark.parametrize("variant", ["base", "truncated"])
@pytest.mark.parametrize("form,k", CACHES, ids=[f"{f.id}-{k}" for f, k in CACHES])
def test_factor_cache_fill_hit_and_misses(form, k, variant):
    """A fill, then a hit with another variable: both bit-identical to the option off with
    record_reuse = 0, the hit by the form's hit kernel alone.  Then one err_muti[v] of SYNOP
    changes, then one is_assim[v] of SOUND: each a miss that equals the option off on the new
    parameters."""
    case = gc.make(variant, k)
    core = dict(weight_function=case.weight_function, q1_mode=case.q1_mode)
    vars_ = variables(case, 2)
    inp, muti, assim = GtsInputs(case), GtsInputs(case), GtsInputs(case)
    muti.vp.gts[abi.GTS_SYNOP - 1].err_muti[2] = 1.5
    assim.vp = copy.deepcopy(muti.vp)
    assim.vp.gts[abi.GTS_SOUND - 1].is_assim[2] = 1
    r = GtsRun(inp, reuse=0, opts=BATCH, base={}, **core)
    try:
        want = [r.call(v)[:2] for v in vars_]
        r.sync(muti)
        want_muti = r.call(vars_[1])[:2]
        r.sync(assim)
        want_assim = r.call(vars_[1])[:2]
    finally:
        r.close()
    same(want[0], plain(variant, k)[:2])
    assert want[0][1]["solved"] > 0
    assert want_muti[1]["nobs_sum"] != want[1][1]["nobs_sum"] or not np.array_equal(
        bits(want_muti[0]), bits(want[1][0]))
    assert want_assim[1]["nobs_sum"] > want_muti[1]["nobs_sum"]
    n = form.names(k)
    r = GtsRun(inp, opts=form.on, base={}, **core)
    try:
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(vars_[0])
        is_miss(info, 3, several=False)
        same((out, cnt), want[0])
        kt = r.c.kernel_times()
        assert n.fill in kt and n.hit not in kt and n.plain not in kt, kt
        assert n.head is None or n.head in kt, kt
        r.c.set_kernel_timing(True)
        out, cnt, info = r.call(vars_[1])
        is_hit(info, 3)
        same((out, cnt), want[1])
        kt = r.c.kernel_times()
        assert sorted(kt) == [n.hit] and kt[n.hit]["points"] == case.points, kt
        for new, ref in ((muti, want_muti), (assim, want_assim)):
            r.sync(new)
            out, cnt, info = r.call(vars_[1])
            is_miss(info, 3, several=False)
            same((out, cnt), ref)
        out, cnt, info = r.call(vars_[1])
        is_hit(info, 3)
        same((out, cnt), want_assim)
    finally:
        r.close()


# ---- column sharing ----------------------------------------------------------------------------
SHARED = [(32, 1), (64, 1), (96, 1), (128, 1), (32, 2)]


@pytest.mark.parametrize("k,share", SHARED, ids=[f"{k}-share{s}" for k, s in SHARED])
def test_column_share_on_flat(k, share):
    """SYNOP and GPSPW alone localise in 2-D: the call runs once per column and equals the
    per-point call bit for bit (12 x 12 = 144 columns, a multiple of 4: exact on the record
    path too), which meets the oracle."""
    case = gc.make("flat", k)
    off, cnt0, _, info0 = plain("flat", k)
    assert info0["shared"] == 0 and info0["reason"] == abi.COLUMN_REASON_OFF, info0
    out, cnt, kt, info = analyse(case, opts={"column_share": share})
    assert info["shared"] == 1 and info["columns"] == case.nx * case.ny, info
    assert info["levels"] == case.nz, info
    assert cnt == cnt0, (cnt, cnt0)
    assert np.array_equal(bits(out), bits(off))
    assert not [n for n in kt if n in kernels_of(k)], kt
    against_oracle(case, off, cnt0, *gc.oracle_ref("flat", k))


def test_column_share_falls_back_with_a_3d_type():
    """The base case: SOUND and VR are 3-D."""
    case = gc.make("base", 96)
    out, cnt, kt, info = analyse(case, opts={"column_share": 1})
    assert info["shared"] == 0 and info["reason"] == abi.COLUMN_REASON_3D, info
    off, cnt0, kt0, _ = plain("base", 96)
    assert cnt == cnt0 and np.array_equal(bits(out), bits(off))
    assert sorted(kt) == sorted(kt0), (kt, kt0)


# ---- device-built index, device-resident obs ---------------------------------------------------
@pytest.mark.parametrize("variant", ["base", "truncated"])
def test_device_index(variant):
    """index = 1: the lists hold obs indices instead of tree slots, times nvar again in the
    stagers; only the column order changes."""
    case = gc.make(variant, 96)
    out, cnt, _, _ = analyse(case, opts={"index": 1})
    off, cnt0, _, _ = plain(variant, 96)
    for name in ORACLE_COUNTERS + ("points", "nonconverged"):
        assert cnt[name] == cnt0[name], (name, cnt, cnt0)
    rel = increment_rel_rms(out, off, case.var)
    print(f"{variant}: index 1 vs index 0 {rel:.3e}")
    assert rel <= 1e-9, rel
    if variant == "truncated":
        assert cnt["lz_truncated"] > 0


def test_device_resident_obs_set():
    """Every obs array in device memory, qc as int32: bit-identical to the host obs set."""
    case = gc.make("base", 96)
    out, cnt, _, _ = analyse(case, memory=abi.MEM_DEVICE)
    off, cnt0, _, _ = plain("base", 96)
    assert cnt == cnt0 and np.array_equal(bits(out), bits(off))
