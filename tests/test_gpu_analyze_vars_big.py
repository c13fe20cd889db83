"""GPU tests of cwbl_analyze_vars on the hand-off path (k = 65..128): one search, one group
hand-off kernel (solve_tq_big_multi_kernel at KP = 96, solve_tq_rows_multi_kernel at KP = 128)
and one solve_tqb_tail_multi_kernel per sub-batch for the whole group.  The kernels assemble
and tridiagonalise once per point and carry every variable's x' through the steps with the
single kernels' expressions, so every comparison with the per-variable calls (`seq`:
cwbl_analyze_var per variable on a fresh core) is exact: np.array_equal on the bit patterns,
plus the counters.  Here only the oracle comparison has a tolerance, the project's
path-versus-oracle bar INCR_TOL, and every input is the benign c2 one (levels 1..3, a single
quadrature pass): the second pass, the fp64 truth and non-finite variables are in
tests/test_gpu_analyze_vars_spectra.py, two obs types, Gaspari-Cohn weights and truncated
lists in tests/test_gpu_analyze_vars_big_mixed.py.

Workloads: synth c2 on 12 x 12 x 5 = 720 points in search batches of at most 256 points (three
batches per call), with 400 obs (every point has p above every k: full-rank Yb Yb^T), with
120 obs (p <= 120: every point rank-deficient at k = 128, exact-zero reflectors with tau = 0;
mixed at k = 65..96), and with every 40th of the 120 (3 obs: points with p = 0).
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, group, same_as_seq, seq, variables

pytestmark = pytest.mark.gpu

INCR_TOL = 1e-6
BATCH = {"max_batch": 256}
GROUP_NAMES = ("solve_tq_rows_multi_kernel<", "solve_tq_big_multi_kernel<",
               "solve_tqb_tail_multi_kernel<")
SINGLE_NAMES = ("solve_tq_rows_kernel<", "solve_tq_big_kernel<", "solve_tqb_tail_kernel<")
SEARCH = "search_binned_kernel"


def opts_of(**more):
    o = dict(BATCH)
    o.update(more)
    return o


@functools.lru_cache(maxsize=None)
def workload(k, n_obs=400):
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=n_obs, k=k)


@functools.lru_cache(maxsize=None)
def seq8(k, n_obs=400):
    """The per-variable analyses of eight variables at ensemble size k, computed once."""
    w = workload(k, n_obs)
    ref = seq(w, variables(w, 8), [w.vp] * 8, opts=opts_of())
    assert ref[0][1]["solved"] == w.points
    return ref


def all_differ(outs):
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not np.array_equal(bits(outs[i]), bits(outs[j])), (i, j)


def names(kt, prefixes):
    return [n for n in kt if n.startswith(prefixes)]


def kp_of(k):
    return 96 if k <= 96 else 128


def group_names(k, nvar):
    """The group head and tail kernel of ensemble size k and group size nvar."""
    nv = 2 if nvar == 2 else 4 if nvar <= 4 else 8
    head = (f"solve_tq_big_multi_kernel<96, 32, {nv}>" if kp_of(k) == 96
            else f"solve_tq_rows_multi_kernel<128, 64, {nv}>")
    return head, f"solve_tqb_tail_multi_kernel<{kp_of(k)}, {kp_of(k) - 64}, {nv}>"


def timed_group(w, nvar, opts):
    lib = Lib(w, opts)
    try:
        lib.c.set_kernel_timing(True)
        got = lib.group(variables(w, nvar), [w.vp] * nvar)
        return got, lib.c.kernel_times()
    finally:
        lib.close()


# KP = 96: k = 65 (the fewest tail steps), 80, 96 (k = KP); KP = 128: k = 97, 100 (padding
# rows), 128 (every lane live)
@pytest.mark.parametrize("n_obs", [400, 120])
@pytest.mark.parametrize("nvar", [2, 8])
@pytest.mark.parametrize("k", [65, 80, 96, 97, 100, 128])
def test_classes_and_padding(k, nvar, n_obs):
    w = workload(k, n_obs)
    ref = seq8(k, n_obs)[:nvar]
    if n_obs == 120:  # p <= 120 < k: no point has a full-rank Yb Yb^T
        assert ref[0][1]["max_p"] <= 120
    got = group(w, variables(w, nvar), [w.vp] * nvar, opts=opts_of())
    same_as_seq(got, ref)
    all_differ(got[0])


@pytest.mark.parametrize("nvar", [3, 5, 7])
@pytest.mark.parametrize("k", [80, 128])
def test_odd_group_size(k, nvar):
    """Slots of a class left empty: 3 of 4, 5 and 7 of 8."""
    w = workload(k)
    got = group(w, variables(w, nvar), [w.vp] * nvar, opts=opts_of())
    same_as_seq(got, seq8(k)[:nvar])
    all_differ(got[0])


@pytest.mark.parametrize("nvar", [2, 3, 8])
@pytest.mark.parametrize("k", [96, 128])
def test_fused_path_taken(k, nvar):
    """One search, one group hand-off kernel and one group tail per batch over all points,
    whatever nvar; no single-variable kernel."""
    w = workload(k)
    got, kt = timed_group(w, nvar, opts_of())
    same_as_seq(got, seq8(k)[:nvar])
    head, tail = group_names(k, nvar)
    assert sorted(names(kt, GROUP_NAMES)) == sorted([head, tail]), kt
    assert not names(kt, SINGLE_NAMES), kt
    assert kt[head]["points"] == w.points and kt[tail]["points"] == w.points, kt
    assert kt[SEARCH]["points"] == w.points, kt  # once, not nvar times
    assert kt[head]["launches"] == kt[tail]["launches"] == kt[SEARCH]["launches"] >= 3, kt


@pytest.mark.parametrize("k", [96, 128])
def test_sub_batches(k):
    """big_batch 128 under max_batch 256: two hand-off sub-batches per search batch."""
    w = workload(k)
    got, kt = timed_group(w, 3, opts_of(big_batch=128))
    same_as_seq(got, seq8(k)[:3])
    head, tail = group_names(k, 3)
    assert kt[head]["points"] == w.points and kt[tail]["points"] == w.points, kt
    assert kt[head]["launches"] == kt[tail]["launches"] == 2 * kt[SEARCH]["launches"], kt


def test_group_of_one_runs_the_single_kernels():
    w = workload(128)
    got, kt = timed_group(w, 1, opts_of())
    same_as_seq(got, seq8(128)[:1])
    assert not names(kt, GROUP_NAMES), kt
    assert len(names(kt, SINGLE_NAMES)) == 2, kt
    assert kt[SEARCH]["points"] == w.points, kt


@pytest.mark.parametrize("k", [96, 128])
def test_sparse(k):
    """Every 40th of the 120 obs (3 obs): points with p = 0, untouched in every variable."""
    wl = copy.copy(workload(k, 120))
    keep = np.arange(wl.obs.shape[0]) % 40 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    vars_ = variables(wl, 3)
    ref = seq(wl, vars_, [wl.vp] * 3, opts=opts_of())
    cnt = ref[0][1]
    print(f"sparse k={k}: solved {cnt['solved']} of {wl.points}, nobs_sum {cnt['nobs_sum']}")
    assert 0 < cnt["solved"] < wl.points
    got = group(wl, vars_, [wl.vp] * 3, opts=opts_of())
    same_as_seq(got, ref)
    for out, var in zip(got[0], vars_):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() == wl.points - cnt["solved"]


def test_per_variable_epilogue():
    """RTPP only, RTPS only, both with tune_q, neither: each variable's own flags and alphas."""
    w = workload(100)
    vps = [copy.deepcopy(w.vp) for _ in range(4)]
    vps[0].use_rtpp, vps[0].rtpp_alpha, vps[0].use_rtps = 1, 0.5, 0
    vps[1].use_rtpp, vps[1].use_rtps, vps[1].rtps_alpha = 0, 1, 0.7
    vps[2].use_rtpp, vps[2].rtpp_alpha, vps[2].use_rtps, vps[2].rtps_alpha = 1, 0.5, 1, 0.7
    vps[2].tune_q = 1
    vps[3].use_rtpp, vps[3].use_rtps = 0, 0
    vars_ = variables(w, 4)
    ref = seq(w, vars_, vps, opts=opts_of())
    # the settings matter: the same variable under another variable's settings differs
    for i, j in ((0, 3), (1, 3), (2, 0)):
        other = seq(w, [vars_[i]], [vps[j]], opts=opts_of())
        assert not np.array_equal(bits(ref[i][0]), bits(other[0][0])), (i, j)
    same_as_seq(group(w, vars_, vps, opts=opts_of()), ref)


def test_staggered():
    w = workload(128)
    vars_ = variables(w, 2)
    ref = seq(w, vars_, [w.vp] * 2, opts=opts_of(), ix_lim=w.nx - 1)
    got = group(w, vars_, [w.vp] * 2, opts=opts_of(), ix_lim=w.nx - 1)
    same_as_seq(got, ref)
    assert got[1]["points"] == (w.nx - 1) * w.ny * w.nz
    for out, var in zip(got[0], vars_):  # the last column is not analysed
        assert np.array_equal(bits(out[..., -1]), bits(var[..., -1]))
        assert not np.array_equal(bits(out), bits(var))


def test_host_slabs():
    """Pageable numpy slabs: equal to the device-slab result."""
    w = workload(128)
    same_as_seq(group(w, variables(w, 3), [w.vp] * 3, opts=opts_of(), host=True),
                seq8(128)[:3])


def test_info_window():
    w = workload(128)
    same_as_seq(group(w, variables(w, 2), [w.vp] * 2, opts=opts_of(info_window=256)),
                seq8(128)[:2])


@pytest.mark.parametrize("k,more", [(128, {"big_path": 0}), (40, {"solver": 1})])
def test_fallbacks_that_remain(k, more):
    """The unsplit k > 64 kernel and the Jacobi solver: the variables one after another."""
    w = workload(k)
    vars_ = variables(w, 2)
    ref = seq(w, vars_, [w.vp] * 2, opts=opts_of(**more))
    assert ref[0][1]["solved"] > 0
    got, kt = timed_group(w, 2, opts_of(**more))
    same_as_seq(got, ref)
    assert not names(kt, GROUP_NAMES), kt
    assert not [n for n in kt if "multi" in n], kt


def test_group_vs_oracle():
    w = workload(128)
    vars_ = variables(w, 3)
    outs, cnt = group(w, vars_, [w.vp] * 3, opts=opts_of())
    ob = abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs, w.hdxb).build()
    for out, var in zip(outs, vars_):
        ref = var.copy()
        ost = abi.Stats()
        rc = oracle().orc_analyze_var(w.k, 0, -5.0, 0, C.byref(ob), C.byref(w.vp),
                                      C.byref(abi.make_slab(w.x, w.y, w.alt, ref)), 16,
                                      C.byref(ost))
        assert rc == 0
        assert cnt["solved"] == ost.solved and cnt["nobs_sum"] == ost.nobs_sum
        rel = increment_rel_rms(out, ref, var)
        moved = np.count_nonzero(bits(ref) != bits(var))
        print(f"increment_rel_rms vs oracle: {rel:.3e} ({moved} analysed values)")
        assert moved > 0
        assert rel <= INCR_TOL, rel
