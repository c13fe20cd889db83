"""GPU tests of the hand-off path (k = 65..128), single call and group, on inputs that are not
benign: two radar types in one obs set (VR, and DBZ under the norain rules, with their own
localisation: two normalisations, two searches), Gaspari-Cohn weighting with its NaN points
(Q8), and truncated neighbour lists (max_lz_pts below the largest p: the k-d tree re-search,
inside the group call's shared search).  The golden driver cases stop at k = 40, so
solve_tq_big_kernel / solve_tq_rows_kernel / solve_tqb_tail_kernel and their group forms see
these radar inputs only here.  Both types have nvar = 1: GTS types with several variables per
obs (and 2-D trees, the Q1 rules, is_assim, QC flags and per-variable err_muti / err_rej) at
k = 41..128 are in tests/test_gpu_gts_large_k.py.

Per case: cwbl_analyze_var against the oracle at INCR_TOL with NaNs at identical positions and
equal solved / nobs_sum / lz_truncated; cwbl_analyze_vars (three variables) against the
per-variable calls bit for bit (NaNs at equal positions, every other bit pattern equal), plus
the counters.  The conditions on the input (rejected DBZ columns, NaN and finite points,
truncated lists) are asserted on the oracle's output alone.

Workload: synth c2 on 12 x 12 x 5 = 720 points, k = 80 (KP = 96) and 128, 300 VR obs (12 km /
3 km) and 200 DBZ obs (8 km / 2 km; every 10th of both in the Gaspari-Cohn case), search
batches of at most 256 points.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, variables

pytestmark = pytest.mark.gpu

INCR_TOL = 1e-6
NORAIN = -5.0
OPTS = {"max_batch": 256}
GROUP_NAMES = ("solve_tq_rows_multi_kernel<", "solve_tq_big_multi_kernel<",
               "solve_tqb_tail_multi_kernel<")
SINGLE_NAMES = ("solve_tq_rows_kernel<", "solve_tq_big_kernel<", "solve_tqb_tail_kernel<")

#: name: (weight_function, max_lz_pts of both types, every n-th obs kept).  With Gaspari-Cohn
#: weights one obs near the edge of the ball (z -> 2, where the fp32 polynomial cancels to a
#: tiny value of either sign) makes a point NaN: with all 500 obs the oracle leaves 610 of the
#: 720 points NaN, with every 10th obs (30 VR, 20 DBZ, p <= 43) about 200, and 520 finite.
CASES = {"two_types": (0, 1000, 1), "gaspari_cohn": (1, 1000, 10), "truncated": (0, 60, 1)}


@functools.lru_cache(maxsize=None)
def workload(k, max_lz, stride):
    """VR from synth c2; DBZ at other places: a third of the obs report norain with every
    member at norain (rejected, :507), a tenth report norain under a raining ensemble (kept
    whatever the departure, :505-506), a few of the others are gross errors (rejected)."""
    w = synth.make("c2", nx=12, ny=12, nz=5, n_obs=300, k=k)
    d = synth.make("c2", nx=12, ny=12, nz=5, n_obs=200, k=k, seed=77)
    rng = np.random.default_rng(k)
    n = d.obs.shape[0]
    dbz_obs = (10.0 + 5.0 * d.obs).astype(np.float32)
    dbz_hdxb = (10.0 + 5.0 * d.hdxb).astype(np.float32)
    kind = rng.uniform(size=n)
    dry = kind < 1 / 3
    dbz_obs[dry] = NORAIN
    dbz_hdxb[:, dry] = NORAIN
    dbz_obs[(kind >= 1 / 3) & (kind < 0.43)] = NORAIN
    dbz_obs[kind > 0.95] += 500.0
    def cut(a, axis=0):
        return np.ascontiguousarray(a.take(np.arange(0, a.shape[axis], stride), axis))

    w.obs_xyz, w.obs, w.hdxb = cut(w.obs_xyz), cut(w.obs), cut(w.hdxb, 1)
    w.dbz = (cut(d.obs_xyz), cut(dbz_obs), cut(dbz_hdxb, 1))
    vr = abi.type_params(use_it=1, max_lz_pts=max_lz, hclr=12.0, vclr=3.0, err_muti=1.0,
                         err_rej=8.0)
    dbz = abi.type_params(use_it=1, max_lz_pts=max_lz, hclr=8.0, vclr=2.0, err_muti=2.5,
                          err_rej=4.0)
    w.vp = abi.var_params(multi_infl=1.6, use_rtpp=1, rtpp_alpha=0.95, use_rtps=1,
                          rtps_alpha=0.95, radar={abi.RADAR_VR: vr, abi.RADAR_DBZ: dbz})
    return w


def obs_set(w):
    return (abi.ObsSetBuilder().add_radar(abi.RADAR_DBZ, *w.dbz)
            .add_radar(abi.RADAR_VR, w.obs_xyz, w.obs, w.hdxb).build())


def oracle_run(w, wf, var):
    ref = var.copy()
    st = abi.Stats()
    ob = obs_set(w)
    rc = oracle().orc_analyze_var(w.k, wf, NORAIN, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, w.alt, ref)), 16, C.byref(st))
    assert rc == 0
    return ref, st


def nan_aware_equal(a, b):
    """NaNs at the same places, every other value equal in its bits."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def vr_only(w):
    """The same call without the DBZ type: what the oracle counts when DBZ adds nothing."""
    vp = copy.deepcopy(w.vp)
    vp.radar[abi.RADAR_DBZ - 1].use_it = 0
    return vp


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("k", [80, 128])
def test_single_and_group_vs_oracle(k, case):
    wf, max_lz, stride = CASES[case]
    w = workload(k, max_lz, stride)
    vars_ = variables(w, 3)
    # ---- the input's conditions, on the oracle alone -----------------------------------------
    ref, ost = oracle_run(w, wf, vars_[0])
    nan_pts = int(np.isnan(ref).any(axis=0).sum())
    moved = np.any(bits(ref) != bits(vars_[0]), axis=0)
    fin_pts = int((moved & ~np.isnan(ref).any(axis=0)).sum())
    # DBZ takes part (other counts than VR alone) and some of its columns are rejected (fewer
    # than a DBZ set without the norain / gross-error obs would add: every point's DBZ ball holds
    # obs of each kind at this density, so nobs_sum falls short of all neighbours)
    w1 = copy.copy(w)
    w1.vp = vr_only(w)
    _, ost_vr = oracle_run(w1, wf, vars_[0])
    assert ost.nobs_sum > ost_vr.nobs_sum
    wide = copy.copy(w)
    wide.vp = copy.deepcopy(w.vp)
    wide.vp.radar[abi.RADAR_DBZ - 1].err_rej[0] = 1e30
    wide.dbz = (w.dbz[0], w.dbz[1], w.dbz[2] + np.float32(0.0))
    wide.dbz[2][0, :] += np.float32(1.0)          # no ensemble sits wholly at norain
    _, ost_all = oracle_run(wide, wf, vars_[0])
    if case != "truncated":
        assert ost_all.nobs_sum > ost.nobs_sum, (ost_all.nobs_sum, ost.nobs_sum)
    print(f"k={k} {case}: oracle solved {ost.solved} nobs_sum {ost.nobs_sum} (VR alone "
          f"{ost_vr.nobs_sum}, no DBZ rejects {ost_all.nobs_sum}) lz_truncated "
          f"{ost.lz_truncated} max_p {ost.max_p}; {nan_pts} NaN points, {fin_pts} finite")
    if case == "gaspari_cohn":
        assert nan_pts >= 5 and fin_pts >= 300, (nan_pts, fin_pts)
    else:
        assert nan_pts == 0 and fin_pts == ost.solved
    if case == "truncated":
        assert ost.lz_truncated > 0 and ost.max_p <= 2 * max_lz
    else:
        assert ost.lz_truncated == 0
    # ---- single calls against the oracle, the group against the single calls ----------------
    lib = Lib(w, OPTS, weight_function=wf, norain_value=NORAIN, obs_set=obs_set(w))
    try:
        lib.c.set_kernel_timing(True)
        singles = [lib.one(v, w.vp) for v in vars_]
        kt1 = dict(lib.c.kernel_times())
        outs, cnt = lib.group(vars_, [w.vp] * 3)
        kt = lib.c.kernel_times()
    finally:
        lib.close()
    assert len([n for n in kt1 if n.startswith(SINGLE_NAMES)]) == 2, kt1
    assert len([n for n in kt if n.startswith(GROUP_NAMES)]) == 2, kt
    for i, (var, (out, scnt)) in enumerate(zip(vars_, singles)):
        oref, st = (ref, ost) if i == 0 else oracle_run(w, wf, var)
        for name in ("solved", "nobs_sum", "lz_truncated"):
            assert scnt[name] == getattr(st, name), (i, name, scnt, getattr(st, name))
        rel = increment_rel_rms(out, oref, var)
        print(f"  variable {i}: single call vs oracle {rel:.3e}, "
              f"{int(np.isnan(out).sum())} NaN values")
        assert rel <= INCR_TOL, (i, rel)
        assert np.array_equal(np.isnan(out), np.isnan(oref))
        assert cnt == scnt, (i, cnt, scnt)
        assert nan_aware_equal(outs[i], out), i
    for i in range(3):
        for j in range(i + 1, 3):
            assert not nan_aware_equal(outs[i], outs[j]), (i, j)
