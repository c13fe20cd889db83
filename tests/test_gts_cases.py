"""The conditions on the input of tests/gts_cases.py, asserted on the oracle alone
(orc_analyze_var, orc_search and numpy; no GPU): each variant holds what it is there for at the
ensemble sizes tests/test_gpu_gts_large_k.py runs it at.  These are conditions, not
measurements: if a seed or a count misses one, the generator changes, not the condition.
"""
import numpy as np
import pytest

import gts_cases as gc
from cwbl import abi

NTREES = {"q1_undef": 3, "sparse": 2, "flat": 2, "nvar3": 5}  # 4 on the mixed base


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("variant", gc.VARIANTS)
@pytest.mark.parametrize("k", [64, 96, 128])
def test_variant_conditions(k, variant):
    case = gc.make(variant, k)
    ref, st = gc.oracle_ref(variant, k)
    nan_pts = int(np.isnan(ref).any(axis=0).sum())
    moved = np.any(bits(ref) != bits(case.var), axis=0)
    fin_pts = int((moved & ~np.isnan(ref).any(axis=0)).sum())
    print(f"k={k} {variant}: ntrees {st.ntrees} solved {st.solved} nobs_sum {st.nobs_sum} "
          f"max_p {st.max_p} lz_truncated {st.lz_truncated} q1_undefined {st.q1_undefined}; "
          f"{nan_pts} NaN points, {fin_pts} finite moved points")
    assert st.points == case.points == 720
    assert st.ntrees == NTREES.get(variant, 4)
    assert (st.lz_truncated > 0) == (variant == "truncated")
    assert (st.q1_undefined > 0) == (variant == "q1_undef")
    if variant == "q1_undef":
        assert st.q1_undefined == case.points      # SYNOP, at every point
    if variant == "gaspari_cohn":
        assert nan_pts > 0 and fin_pts >= 300, (nan_pts, fin_pts)
    else:
        assert nan_pts == 0 and fin_pts == st.solved
    if variant == "sparse":
        assert 0 < st.solved < case.points and st.nobs_sum / st.solved < k
    else:
        assert st.solved == case.points
    if variant == "dense":
        assert st.nobs_sum / st.solved > 500       # several chunks of 64 per tree
    if variant == "per_type":                      # the mode matters on this input
        assert st.nobs_sum < gc.oracle_ref("base", k)[1].nobs_sum
    if variant == "nvar3":                         # the three-variable type takes part
        assert st.nobs_sum > gc.oracle_ref("base", k)[1].nobs_sum


@pytest.mark.parametrize("variant", gc.VARIANTS)
def test_accept_rules_remove_columns(variant):
    """The gross-error and QC rules remove columns, and so does is_assim (SOUND or SYNOP, each
    with one zero there, is in every variant)."""
    case = gc.make(variant, 96)
    _, st = gc.oracle_ref(variant, 96)
    _, st_all = gc.oracle_run(gc.no_rejects(case), case.var)
    assert st_all.nobs_sum > st.nobs_sum, (st_all.nobs_sum, st.nobs_sum)
    _, st_assim = gc.oracle_run(gc.all_assimilated(case), case.var)
    assert st_assim.nobs_sum > st.nobs_sum, (st_assim.nobs_sum, st.nobs_sum)


@pytest.mark.parametrize("variant", [v for v in gc.VARIANTS if v != "sparse"])
def test_chunks_cut_through_an_observation(variant):
    """Some point's (obs, variable) pair count of a five-variable type exceeds 64 and is a
    multiple of neither 32 nor 64: on every stager (chunks of 32 or 64 pairs) chunk boundaries
    fall inside observations and the last chunk is partial.  (Under `truncated` the search keeps
    six of these neighbours: the count here is the ball's.)"""
    case = gc.make(variant, 96)
    five = [tid for tid in case.gts if gc.GTS[tid][0] == 5]
    assert five
    for tid in five:
        n = gc.pair_counts(case, tid)
        hit = (n > 64) & (n % 32 != 0)
        print(f"{variant} type {tid}: up to {n.max()} pairs, {int(hit.sum())} points qualify")
        assert hit.any()


def test_layouts_and_classes():
    """add_gts's layouts, and the QC classes of the columns: dropped, partly flagged, clean."""
    case = gc.make("base", 96)
    for tid, (xyz, obs, error, hdxb, qc) in case.gts.items():
        nvar = gc.GTS[tid][0]
        n = xyz.shape[0]
        assert xyz.shape == (n, 3) and obs.shape == error.shape == (n, nvar)
        assert hdxb.shape == qc.shape == (96, n, nvar)
        assert qc.dtype == np.int32 and hdxb.dtype == obs.dtype == np.float32
        assert 0.5 <= error.min() and error.max() <= 2.0
        dropped = (qc < 0).all(axis=0)
        partly = (qc < 0).any(axis=0) & ~dropped
        assert dropped.any() and partly.any() and (~dropped & ~partly).any()
    sound = case.vp.gts[abi.GTS_SOUND - 1]
    synop = case.vp.gts[abi.GTS_SYNOP - 1]
    assert list(sound.is_assim)[:4].count(0) == 1 and list(synop.is_assim).count(0) == 1
    assert len(set(sound.err_muti[:4])) == 4 and len(set(synop.err_rej)) == 5
    assert sound.vclr > 0 and synop.vclr < 0
