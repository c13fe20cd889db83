"""GPU tests of cwbl_analyze_vars on the one-wavefront path (k <= 16, k = 41..64, and
k = 17..40 with split40 = 0): one search and one solve_tq_multi_kernel per batch for the whole
group.  The kernel tridiagonalises once per point and carries every variable's x' through the
steps with solve_tq_kernel's expressions, so every comparison with the per-variable calls
(`seq`: cwbl_analyze_var per variable on a fresh core) is exact: np.array_equal on the bit
patterns, plus the counters.  Here only the oracle comparison has a tolerance, the project's
path-versus-oracle bar INCR_TOL, and every input is the benign c2 one (levels 1..3, a single
quadrature pass): the second pass, the fp64 truth, non-finite variables and the reference's
mixed-obs cases are in tests/test_gpu_analyze_vars_spectra.py and
tests/test_gpu_analyze_vars_golden.py.

Workload: synth c2 on 12 x 12 x 5 = 720 points with 120 obs, in search batches of at most 256
points, so a call runs three batches (the search of one overlaps the solve of the one before).
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits, counters, group, same_as_seq, seq, variables

pytestmark = pytest.mark.gpu

INCR_TOL = 1e-6
BATCH = {"max_batch": 256}
GROUP = "solve_tq_multi_kernel<"
SINGLE = "solve_tq_kernel<"
SEARCH = "search_binned_kernel"


def opts_of(split40=None, **more):
    o = dict(BATCH)
    if split40 is not None:
        o["split40"] = split40
    o.update(more)
    return o


@functools.lru_cache(maxsize=None)
def workload(k):
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)


@functools.lru_cache(maxsize=None)
def seq8(k, split40=None):
    """The per-variable analyses of eight variables at ensemble size k, computed once."""
    w = workload(k)
    ref = seq(w, variables(w, 8), [w.vp] * 8, opts=opts_of(split40))
    assert ref[0][1]["solved"] > 0
    return ref


def all_differ(outs):
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not np.array_equal(bits(outs[i]), bits(outs[j])), (i, j)


# every KP class (8 .. 64), k < KP padding rows (13, 25, 41, 50), k = KP (8, 16, 40, 64: at 64
# all lanes are live) and KP = 40's 2x2 trailing phase
CLASSES = [(8, None), (13, None), (16, None), (41, None), (50, None), (64, None), (25, 0),
           (40, 0)]


@pytest.mark.parametrize("nvar", [2, 8])
@pytest.mark.parametrize("k,split40", CLASSES)
def test_classes_and_padding(k, split40, nvar):
    w = workload(k)
    got = group(w, variables(w, nvar), [w.vp] * nvar, opts=opts_of(split40))
    same_as_seq(got, seq8(k, split40)[:nvar])
    all_differ(got[0])


@pytest.mark.parametrize("nvar", [3, 5, 7])
@pytest.mark.parametrize("k", [13, 64])
def test_odd_group_size(k, nvar):
    """Slots of a class left empty: 3 of 4, 5 and 7 of 8."""
    w = workload(k)
    got = group(w, variables(w, nvar), [w.vp] * nvar, opts=opts_of())
    same_as_seq(got, seq8(k)[:nvar])
    all_differ(got[0])


def timed_group(w, nvar, opts):
    lib = Lib(w, opts)
    try:
        lib.c.set_kernel_timing(True)
        got = lib.group(variables(w, nvar), [w.vp] * nvar)
        return got, lib.c.kernel_times()
    finally:
        lib.close()


@pytest.mark.parametrize("nvar", [2, 3, 8])
@pytest.mark.parametrize("k", [16, 64])
def test_fused_path_taken(k, nvar):
    """One search and one group solve per batch over all points, whatever nvar; no
    per-variable kernel."""
    w = workload(k)
    got, kt = timed_group(w, nvar, opts_of())
    same_as_seq(got, seq8(k)[:nvar])
    fused = [n for n in kt if n.startswith(GROUP)]
    assert len(fused) == 1, kt
    nv = 2 if nvar == 2 else 4 if nvar <= 4 else 8  # the kernel's class of group sizes
    assert fused[0] == f"solve_tq_multi_kernel<{k}, {nv}>", kt  # (k = KP at 16 and 64)
    assert not [n for n in kt if n.startswith(SINGLE)], kt
    assert kt[fused[0]]["points"] == w.points, kt
    assert kt[SEARCH]["points"] == w.points, kt  # once, not nvar times
    assert kt[fused[0]]["launches"] == kt[SEARCH]["launches"] >= 3, kt  # one per batch


@pytest.mark.parametrize("k", [16, 64])
def test_group_of_one_runs_the_single_kernel(k):
    w = workload(k)
    got, kt = timed_group(w, 1, opts_of())
    same_as_seq(got, seq8(k)[:1])
    assert not [n for n in kt if n.startswith(GROUP)], kt
    assert [n for n in kt if n.startswith(SINGLE)], kt
    assert kt[SEARCH]["points"] == w.points, kt


@pytest.mark.parametrize("k", [16, 64])
def test_sparse(k):
    """Every 40th obs (3 of 120; every 10th still reaches all 720 points): points with p = 0
    (untouched in every variable) and with p < k (rank-deficient Yb Yb^T: exactly-zero
    reflectors, tau = 0)."""
    wl = copy.copy(workload(k))
    keep = np.arange(wl.obs.shape[0]) % 40 == 0
    wl.obs_xyz = np.ascontiguousarray(wl.obs_xyz[keep])
    wl.obs = np.ascontiguousarray(wl.obs[keep])
    wl.hdxb = np.ascontiguousarray(wl.hdxb[:, keep])
    vars_ = variables(wl, 3)
    ref = seq(wl, vars_, [wl.vp] * 3, opts=opts_of())
    cnt = ref[0][1]
    print(f"sparse k={k}: solved {cnt['solved']} of {wl.points}, nobs_sum {cnt['nobs_sum']}")
    assert 0 < cnt["solved"] < wl.points
    assert cnt["nobs_sum"] / cnt["solved"] < k
    got = group(wl, vars_, [wl.vp] * 3, opts=opts_of())
    same_as_seq(got, ref)
    for out, var in zip(got[0], vars_):
        untouched = np.all(bits(out) == bits(var), axis=0)
        assert untouched.sum() == wl.points - cnt["solved"]


def test_per_variable_epilogue():
    """RTPP only, RTPS only, both with tune_q, neither: each variable's own flags and alphas."""
    w = workload(50)
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
    w = workload(64)
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
    w = workload(64)
    same_as_seq(group(w, variables(w, 3), [w.vp] * 3, opts=opts_of(), host=True), seq8(64)[:3])


def test_info_window():
    w = workload(64)
    same_as_seq(group(w, variables(w, 2), [w.vp] * 2, opts=opts_of(info_window=256)),
                seq8(64)[:2])


def test_group_vs_oracle():
    w = workload(64)
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


@pytest.mark.parametrize("k,more", [(128, {}), (40, {"solver": 1})])
def test_fallbacks_that_remain(k, more):
    """k > 64 and the Jacobi solver: the variables one after another, as before."""
    w = workload(k)
    vars_ = variables(w, 2)
    ref = seq(w, vars_, [w.vp] * 2, opts=opts_of(**more))
    assert ref[0][1]["solved"] > 0
    got, kt = timed_group(w, 2, opts_of(**more))
    same_as_seq(got, ref)
    assert not [n for n in kt if n.startswith(GROUP)], kt
