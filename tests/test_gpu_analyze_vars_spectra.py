"""GPU tests of cwbl_analyze_vars on wide spectra and with a non-finite variable: every
quadrature rule of every group kernel (solve_tq40_multi_kernel's 15-, 23-, 31- and 63-node
rounds, both passes of solve_tq_multi_kernel and of solve_tqb_tail_multi_kernel<96|128>, each
run once per variable inside the kernels' variable loop), pinned three ways:

 * bit for bit against the per-variable cwbl_analyze_var calls, counters included;
 * the level counters (max_sweeps, sweeps_sum) against the level map the CPU computes from
   the fp64 spectrum bound (tests/spectra_cases.py), which also shows, without the GPU, that the
   intended R / pass classes and the mixed groups of four are in the input;
 * variable 0 against the fp64 truth (helpers.eigen_direct_solve) at every point, and against
   the oracle where every level of the case is below 13.

Only variable 0 carries the pair ensemble; variables 1.. are `variables()`' N(0,1) noise on it.
They are held to bit-identity with their own single calls alone, never to the truth, so the
floor condition of the truth bound (spectra_cases.Case.tol) does not bear on them.

Tolerances.  Truth: max(tol INCR_TOL, ulp), ulp the fp32 rounding floor of the increments.
tol = 1 except in the sparse 2^-18 cases (p = 3..12 < k), whose fp64 floor (the truth
evaluated with the columns reversed, measured on the CPU) is 1.13e-6 at k = 16, 2.55e-5 at 32,
3.58e-5 at 64, 7.23e-5 at 96 and 9.39e-5 at 128 (the oracle's own deviation from the truth
there: 6.9e-6, 3.0e-5, 5.1e-5, 8.0e-5, 1.1e-4): tol is the smallest integer >= 4 x floor /
INCR_TOL = 5, 103, 144, 290, 376 (spectra_cases.SPARSE_TOL; tests/test_truth_spectra.py holds
the floors to it).  Oracle: INCR_TOL, only for cases whose levels all lie below 13: the
oracle forms Pa and multiplies it by Yb d, and at levels 11 and 12 it is itself 1.7e-6 ..
7.3e-6 from the truth on these workloads (printed per case as rel_ref), at 13 and above 1e-4.

The closed-form spectrum A = inflat I + diag(4^e) of test_quadrature_on_an_exact_wide_spectrum
cannot be reached through cwbl_analyze_vars: obs_prep_kernel subtracts the member mean, so
every column of Yb sums to zero over the members and Yb^T Yb is never diagonal.  The case here
uses the nearest exact form instead, one obs per member pair (column i = +-2^e_i on members 2i,
2i + 1, mean exactly 0): A is block diagonal in 2 x 2 blocks, already tridiagonal, with
eigenvalues inflat and inflat + 2 4^e_i, and the analysis is known in closed form.
"""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest

import spectra_cases as sc
from cwbl import abi, synth
from helpers import increment_rel_rms, inflat_of, oracle, quad_level
from test_gpu_analyze_vars import Lib, bits, group, same_as_seq, seq, variables

pytestmark = pytest.mark.gpu

INCR_TOL = sc.INCR_TOL
RECORD_OPTS = {"max_batch": 256, "split40_batch": 128, "record_reuse": 0}
OTHER_OPTS = {"max_batch": 256}


def opts_of(k):
    return RECORD_OPTS if sc.on_record_path(k) else OTHER_OPTS


def fused_names(k, kt):
    """The group kernels of ensemble size k among the timed kernels; no single-variable
    solve kernel may have run."""
    if sc.on_record_path(k):
        want, single = ("solve_tq40_multi_kernel<",), ("solve_tq40_kernel<",)
    elif k <= 64:
        want, single = ("solve_tq_multi_kernel<",), ("solve_tq_kernel<",)
    else:
        want = ("solve_tq_rows_multi_kernel<" if k > 96 else "solve_tq_big_multi_kernel<",
                "solve_tqb_tail_multi_kernel<")
        single = ("solve_tq_rows_kernel<", "solve_tq_big_kernel<", "solve_tqb_tail_kernel<")
    got = sorted(n for n in kt if n.startswith(want))
    assert len(got) == len(want), kt
    assert not [n for n in kt if n.startswith(single)], kt
    return got


def timed_group(w, vars_, vps, opts):
    lib = Lib(w, opts)
    try:
        lib.c.set_kernel_timing(True)
        got = lib.group(vars_, vps)
        return got, lib.c.kernel_times()
    finally:
        lib.close()


def all_differ(outs):
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not np.array_equal(bits(outs[i]), bits(outs[j])), (i, j)


def check_levels(c, ev, cnt):
    """The input conditions (no GPU) and the call's level counters against the level map."""
    lv = ev.levels
    assert ev.near.sum() == 0
    present = sc.classes_present(c, lv)
    assert present == sorted(c.classes), present
    mixed = sc.mixed_fours(c, lv)
    assert (mixed > 0) == c.mixed, mixed
    assert cnt["nonconverged"] == 0
    assert cnt["solved"] == np.count_nonzero(lv)
    assert cnt["max_sweeps"] == lv.max(), (cnt["max_sweeps"], lv.max())
    assert abs(cnt["sweeps_sum"] - int(lv.sum())) <= ev.near.sum(), (cnt["sweeps_sum"], lv.sum())
    return present, mixed


def check_truth(c, w, ev, out):
    """Variable 0 of the group against the fp64 truth and, where it is accurate, the oracle."""
    ulp = sc.ulp_floor(ev.truth, w.var)
    rel = increment_rel_rms(out, ev.truth, w.var)
    ref = w.var.copy()
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    ost = abi.Stats()
    rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                  C.byref(abi.make_slab(w.x, w.y, w.alt, ref)), 16,
                                  C.byref(ost))
    assert rc == 0
    rel_ref = increment_rel_rms(ref, ev.truth, w.var)
    rel_orc = increment_rel_rms(out, ref, w.var)
    print(f"  vs truth {rel:.3e} (bound {max(c.tol * INCR_TOL, ulp):.3e}, ulp {ulp:.3e}), "
          f"oracle vs truth rel_ref {rel_ref:.3e}, vs oracle {rel_orc:.3e}")
    assert rel <= max(c.tol * INCR_TOL, ulp), (rel, ulp, rel_ref)
    if ev.levels.max() < 13:
        assert rel_orc <= max(INCR_TOL, ulp), (rel_orc, ulp)
    return ost


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_every_rule_in_a_group_of_three(c):
    w = sc.workload(c)
    assert sc.means_exact(w)
    ev = sc.evaluate(c)
    vars_ = variables(w, 3)
    vps = [w.vp] * 3
    ref = seq(w, vars_, vps, opts=opts_of(c.k))
    got, kt = timed_group(w, vars_, vps, opts_of(c.k))
    same_as_seq(got, ref)
    all_differ(got[0])
    present, mixed = check_levels(c, ev, got[1])
    u, n = np.unique(ev.levels, return_counts=True)
    print(f"{sc.case_id(c)}: {fused_names(c.k, kt)} levels {dict(zip(u.tolist(), n.tolist()))} "
          f"{'R' if sc.on_record_path(c.k) else 'passes'} {present}, {mixed} mixed fours")
    ost = check_truth(c, w, ev, got[0][0])
    assert got[1]["solved"] == ost.solved and got[1]["nobs_sum"] == ost.nobs_sum


def epilogues(vp):
    """Eight variables' settings: RTPP only (the pair ensemble's), neither, other alphas.
    RTPS stays off at these levels (helpers.pair_ensemble)."""
    out = []
    for on, alpha in ((1, 0.95), (0, 0.95), (1, 0.5), (1, 0.25), (1, 0.75), (0, 0.5), (1, 0.125),
                      (1, 0.875)):
        v = copy.deepcopy(vp)
        v.use_rtpp, v.rtpp_alpha, v.use_rtps = on, alpha, 0
        out.append(v)
    return out


@pytest.mark.parametrize("c", [c for c in sc.CASES if c.n_obs > 12 and c.e == -19],
                         ids=sc.case_id)
def test_eight_variables_with_their_own_epilogues_at_the_63_node_rule(c):
    """Levels 13 and above (R = 8, two passes) in every point: the quadrature result feeds each
    variable's own epilogue, so a slot mix-up between variables shows."""
    w = sc.workload(c)
    ev = sc.evaluate(c)
    assert ev.levels.min() >= 13
    vars_ = variables(w, 8)
    vps = epilogues(w.vp)
    ref = seq(w, vars_, vps, opts=opts_of(c.k))
    # the settings matter: the same variable under another variable's settings differs
    for i, j in ((0, 1), (2, 3), (7, 6)):
        other = seq(w, [vars_[i]], [vps[j]], opts=opts_of(c.k))
        assert not np.array_equal(bits(ref[i][0]), bits(other[0][0])), (i, j)
    got, kt = timed_group(w, vars_, vps, opts_of(c.k))
    same_as_seq(got, ref)
    all_differ(got[0])
    present, _ = check_levels(c, ev, got[1])
    print(f"{sc.case_id(c)} x 8: {fused_names(c.k, kt)} "
          f"{'R' if sc.on_record_path(c.k) else 'passes'} {present}")
    check_truth(c, w, ev, got[0][0])


# ---- the exact block spectrum, and a spectrum beyond the last table ----------------------------
def block_workload(k, emax, seed):
    """One analysed point with k / 2 radar obs at it (r^2 = 0, err 1: weight exactly 1), obs i
    seen by members 2i, 2i + 1 as +-2^e_i and by no other member; three more points 1000 km
    away (p = 0).  Returns (workload, closed-form analysis of `variables`' first variable)."""
    rng = np.random.default_rng(seed)
    h = k // 2
    e = np.round(np.linspace(0, emax, h)).astype(int)
    rng.shuffle(e)
    sgn = rng.choice([-1.0, 1.0], h)
    hdxb = np.zeros((k, h), np.float32)
    hdxb[2 * np.arange(h), np.arange(h)] = sgn * 2.0 ** e
    hdxb[2 * np.arange(h) + 1, np.arange(h)] = -sgn * 2.0 ** e
    yo = (np.round(rng.standard_normal(h) * 64) / 64).astype(np.float32)
    x = np.array([[0.0, 1e6], [0.0, 1e6]], np.float32)
    y = np.array([[0.0, 0.0], [1e6, 1e6]], np.float32)
    alt = np.full((1, 2, 2), 1000.0, np.float32)
    # three variables, members 2i, 2i + 1 = mean +- delta_i on a dyadic grid: x' has no part in
    # the pairs' symmetric directions, whose eigenvalue inflat next to 2 4^e no fp64
    # factorisation of A resolves (helpers.pair_ensemble)
    dy = lambda a: (np.round(np.asarray(a) * 256.0) / 256.0).astype(np.float32)  # noqa: E731
    pm = np.where(np.arange(k) % 2 == 0, 1.0, -1.0).reshape(k, 1, 1, 1)
    vars_ = [np.ascontiguousarray(dy(dy(3.0 + rng.standard_normal((1, 2, 2)))[None] + pm * np.repeat(
        dy(rng.standard_normal((h, 1, 2, 2))), 2, axis=0))) for _ in range(3)]
    var = vars_[0]
    vp = synth.radar_var_params(12.0, 3.0, 1000, 1.0, 8.0, abi.RADAR_VR)
    vp.use_rtpp = vp.use_rtps = 0
    w = types.SimpleNamespace(k=k, x=x, y=y, alt=alt, var=var, vp=vp, radar_type=abi.RADAR_VR,
                              obs_xyz=np.tile(np.array([[0.0, 0.0, 1000.0]], np.float32), (h, 1)),
                              obs=yo, hdxb=hdxb, points=4, vars=vars_)
    return w, e, sgn


def block_closed_form(k, xb, yo, e, sgn, infl):
    """xa of A = inflat I + sum_i 4^e_i (e_2i - e_2i+1)(e_2i - e_2i+1)^T: per pair the symmetric
    direction has eigenvalue inflat, the antisymmetric one lam_i = inflat + 2 4^e_i."""
    s = np.float32(0.0)
    for v in xb:
        s = np.float32(s + v)
    xm = float(np.float32(s * np.float32(1.0 / k)))
    xp = xb.astype(np.float64) - xm
    lam = float(infl) + 2.0 * 4.0 ** e
    assert np.all(lam - 2.0 * 4.0 ** e == float(infl))           # exact in fp64
    sy, an = (xp[0::2] + xp[1::2]) / 2.0, (xp[0::2] - xp[1::2]) / 2.0
    assert np.all(sy == 0.0)                                      # the fp32 mean is exact
    dot = float(np.sum(yo.astype(np.float64) * sgn * 2.0 ** e * 2.0 * an / lam))
    wx = np.empty(k)
    wx[0::2] = sy / np.sqrt(float(infl)) + an / np.sqrt(lam)
    wx[1::2] = sy / np.sqrt(float(infl)) - an / np.sqrt(lam)
    return (xm + (dot + np.sqrt(k - 1.0) * wx)).astype(np.float32), lam


@pytest.mark.parametrize("k", [32, 16, 64, 96, 128])
def test_exact_block_spectrum_through_the_group_call(k):
    """M/m ~ 1e13: R = 8 resp. the second pass on a spectrum whose analysis is known exactly;
    every variable of a group of three against its closed form to 2 fp32 ulps."""
    w, e, sgn = block_workload(k, 24, k)
    infl = inflat_of(k, w.vp.multi_infl)
    vars_ = w.vars
    vps = [w.vp] * 3
    ref = seq(w, vars_, vps, opts=opts_of(k))
    got = group(w, vars_, vps, opts=opts_of(k))
    same_as_seq(got, ref)
    cnt = got[1]
    ratio = 1.0 + float(np.sum(2.0 * 4.0 ** e)) / float(infl)
    assert cnt["solved"] == 1 and cnt["nobs_sum"] == k // 2 and cnt["nonconverged"] == 0, cnt
    assert cnt["max_sweeps"] == quad_level(ratio) >= 13, (cnt, ratio)
    for out, var in zip(got[0], vars_):
        exact, _ = block_closed_form(k, var[:, 0, 0, 0], w.obs, e, sgn, infl)
        err = np.max(np.abs(out[:, 0, 0, 0].astype(np.float64) - exact))
        print(f"k={k}: max |xa - closed form| = {err:.3e}")
        assert err <= 2 * np.spacing(np.float32(8.0)), out[:, 0, 0, 0] - exact
        assert increment_rel_rms(out[:, 0, 0, 0], exact, var[:, 0, 0, 0]) <= INCR_TOL
        far = np.ones((1, 2, 2), bool)
        far[0, 0, 0] = False
        assert np.array_equal(bits(out[:, far]), bits(var[:, far]))   # p = 0: untouched


@pytest.mark.parametrize("k", [32, 16, 64, 96, 128])
def test_spectrum_beyond_the_last_table(k):
    """M/m > 1e24: the kernels run the last table and report the point with a negative level
    (info.y), counted in nonconverged; the group call reports it once, as a single call does."""
    w, e, _ = block_workload(k, 46, k)
    ratio = 1.0 + float(np.sum(2.0 * 4.0 ** e)) / float(inflat_of(k, w.vp.multi_infl))
    assert ratio > 1e25
    vars_ = w.vars
    ref = seq(w, vars_, [w.vp] * 3, opts=opts_of(k))
    got = group(w, vars_, [w.vp] * 3, opts=opts_of(k))
    cnt = got[1]
    assert cnt["solved"] == 1 and cnt["nonconverged"] == 1 and cnt["max_sweeps"] == 24, cnt
    for (out, (single, scnt)) in zip(got[0], ref):
        assert cnt == scnt
        assert nan_aware_equal(out, single)


# ---- a variable that already holds NaN or Inf --------------------------------------------------
def nan_aware_equal(a, b):
    """NaNs at the same places, every other value equal in its bits."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


NAN_POINTS = (7, 130, 255, 256, 511)
INF_POINTS = (3, 257, 400, 640, 719)


def poisoned(var):
    """NaN in every member at five points, +Inf in one member at five others."""
    k = var.shape[0]
    out = var.copy()
    flat = out.reshape(k, -1)
    for g in NAN_POINTS:
        flat[:, g] = np.nan
    for g in INF_POINTS:
        flat[g % k, g] = np.inf
    return out


@functools.lru_cache(maxsize=None)
def benign(k):
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)


@functools.lru_cache(maxsize=None)
def benign_seq8(k):
    w = benign(k)
    return seq(w, variables(w, 8), [w.vp] * 8, opts=opts_of(k))


@functools.lru_cache(maxsize=None)
def benign_group(k, nvar):
    w = benign(k)
    return group(w, variables(w, nvar), [w.vp] * nvar, opts=opts_of(k))


# the slot of variable i: 0 and 1 ride in the first wave_sum4_dpp of a step (1 in its fourth
# value), 2..5 in the second, 6 and 7 in the third: the last slots are 1, 3 (of four), 5 and 7
@pytest.mark.parametrize("nvar,slot", [(2, 1), (4, 3), (4, 1), (8, 7), (8, 5), (8, 1)])
@pytest.mark.parametrize("k", [32, 16, 64, 96, 128])
def test_a_non_finite_variable_stays_in_its_slot(k, nvar, slot):
    w = benign(k)
    assert w.points == 720
    vars_ = variables(w, nvar)
    vars_[slot] = poisoned(vars_[slot])
    clean = benign_seq8(k)
    single = seq(w, [vars_[slot]], [w.vp], opts=opts_of(k))[0]
    bad = ~np.isfinite(single[0])
    hit = np.any(bad, axis=0).ravel()
    assert hit[list(NAN_POINTS + INF_POINTS)].all() and hit.sum() == 10, np.where(hit)[0]
    outs, cnt = group(w, vars_, [w.vp] * nvar, opts=opts_of(k))
    for i, out in enumerate(outs):
        if i == slot:
            assert np.array_equal(~np.isfinite(out), bad)
            assert nan_aware_equal(out, single[0])
            assert np.array_equal(bits(out)[~bad], bits(single[0])[~bad])
        else:
            assert np.array_equal(bits(out), bits(clean[i][0])), i
    assert cnt == single[1] == clean[0][1] == benign_group(k, nvar)[1], (cnt, single[1])
    print(f"k={k}: variable {slot} of {nvar} non-finite at {int(bad.sum())} values of 10 points; "
          f"the other {nvar - 1} bit-identical to their single calls")
