"""GPU tests of the record cache of the k = 17..40 path (CWBL_OPT_RECORD_REUSE, cwbl_reuse_info).

A call whose obs set, options, type parameters, multi_infl, slab shape and coordinates equal
the previous call's solves from the records that call assembled.  The hit feeds the same
record bits to the same kernel, so every comparison here is exact (np.array_equal on the bit
patterns): no tolerance is involved.  Every test checks through reuse_info that the calls it
takes for hits were hits and the ones it takes for misses were misses.

Workload: synth c2 at scale 0.1 (30 x 30 x 50 points, k = 40, 225 obs) in search batches of
1024 points and record sub-batches of 512, i.e. 44 batches of two sub-batches each.
"""
import numpy as np
import pytest

from cwbl import abi, synth
from reuse_harness import Inputs, Run, bits, is_hit, is_miss, no_reuse, other_var, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REC_BYTES = 6880  # AsmRecord<40>: 860 fp64 words


@pytest.fixture(scope="module")
def w():
    return synth.make("c2", scale=0.1)


def test_hit_equals_no_reuse(w):
    """Default budget (reuse is on without any option): the fill, a hit on the same variable
    and a hit on another variable each equal the analysis without reuse, counters included."""
    inp = Inputs(w)
    var2 = other_var(w, 7)
    ref1, ref2 = no_reuse(inp, [w.var, var2])
    assert ref1[1]["solved"] > 0 and not np.array_equal(bits(ref1[0]), bits(ref2[0]))
    r = Run(inp)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info)
        nbat = info["batches_assembled"]
        assert nbat == 44
        # every batch's records and its spare one, the accepted counts, the snapshot
        assert info["bytes_held"] >= (w.points + nbat) * REC_BYTES + 8 * w.points
        same((out, cnt), ref1)
        out, cnt, info = r.call(w.var)
        is_hit(info, nbat)
        same((out, cnt), ref1)
        out, cnt, info = r.call(var2)
        is_hit(info, nbat)
        same((out, cnt), ref2)
    finally:
        r.close()


def test_hit_with_changed_epilogue(w):
    """RTPP / RTPS, their alphas and tune_q act in the solve only: changing them keeps the
    hit, and the result is the no-reuse analysis under the new settings."""
    inp = Inputs(w)
    new = Inputs(w)
    new.vp.use_rtpp, new.vp.rtpp_alpha = 0, 0.5
    new.vp.use_rtps, new.vp.rtps_alpha = 1, 0.7
    new.vp.tune_q = 1
    ref_old, = no_reuse(inp, [w.var])
    ref_new, = no_reuse(new, [w.var])
    assert not np.array_equal(bits(ref_old[0]), bits(ref_new[0]))
    r = Run(inp)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info)
        nbat = info["batches_assembled"]
        same((out, cnt), ref_old)
        r.sync(new)
        out, cnt, info = r.call(w.var)
        is_hit(info, nbat)
        same((out, cnt), ref_new)
    finally:
        r.close()


def _new_hdxb(inp, w):
    rng = np.random.default_rng(5)
    inp.hdxb = (w.hdxb + rng.standard_normal(w.hdxb.shape, dtype=np.float32)).astype(np.float32)


def _new_alt(inp, w):
    inp.alt += np.float32(37.0)


def _new_x(inp, w):
    inp.x += np.float32(500.0)


def _hclr(inp, w):
    inp.tp.hclr = 10.0


def _multi_infl(inp, w):
    inp.vp.multi_infl = 1.1


def _err_muti(inp, w):
    inp.tp.err_muti[0] = 2.0


def _err_rej(inp, w):
    inp.tp.err_rej[0] = 1.0


def _ix_lim(inp, w):
    inp.ix_lim = w.nx - 1


def _bin_div(inp, w):
    inp.options = {"bin_div": 2}


CHANGES = {"set_obs_hdxb": _new_hdxb, "alt_in_place": _new_alt, "x_in_place": _new_x,
           "hclr": _hclr, "multi_infl": _multi_infl, "err_muti": _err_muti, "err_rej": _err_rej,
           "ix_lim": _ix_lim, "bin_div": _bin_div}
# bin_div = 2 is what the density rule picks here anyway, so that case changes no result
CHANGES_RESULT = set(CHANGES) - {"bin_div"}


@pytest.mark.parametrize("what", sorted(CHANGES))
def test_invalidation(w, what):
    """After a fill and a hit, one input of the record changes: the next call is a miss and
    equals the no-reuse analysis of the new inputs (and the call after it hits again)."""
    inp, new = Inputs(w), Inputs(w)
    CHANGES[what](new, w)
    ref_old, = no_reuse(inp, [w.var])
    ref_new, = no_reuse(new, [w.var])
    if what in CHANGES_RESULT:
        assert not np.array_equal(bits(ref_old[0]), bits(ref_new[0]))
    if what == "err_rej":  # some obs are rejected now
        assert ref_new[1]["nobs_sum"] < ref_old[1]["nobs_sum"]
    r = Run(inp)
    try:
        _, _, info = r.call(w.var)
        is_miss(info)
        nbat = info["batches_assembled"]
        out, cnt, info = r.call(w.var)
        is_hit(info, nbat)
        same((out, cnt), ref_old)
        r.sync(new)
        out, cnt, info = r.call(w.var)
        is_miss(info)
        same((out, cnt), ref_new)
        nbat = info["batches_assembled"]
        out, cnt, info = r.call(w.var)
        is_hit(info, nbat)
        same((out, cnt), ref_new)
    finally:
        r.close()


def _ragged_cases():
    yield "k25", synth.make("c2", scale=0.1, k=25)
    yield "k33", synth.make("c2", scale=0.1, k=33)
    # 6 293 points: sub-batches that are no multiple of four, the last wave's lanes past the
    # launch read the spare record (test_split_kp40_ragged_record_batches' slab)
    yield "spare", synth.make("c2", seed=11, nx=31, ny=29, nz=7, n_obs=240)
    thin = synth.make("c2", scale=0.1)
    keep = np.arange(thin.obs.shape[0]) % 25 == 0
    thin.obs_xyz = np.ascontiguousarray(thin.obs_xyz[keep])
    thin.obs = np.ascontiguousarray(thin.obs[keep])
    thin.hdxb = np.ascontiguousarray(thin.hdxb[:, keep])
    yield "sparse", thin


@pytest.mark.parametrize("case", ["k25", "k33", "spare", "sparse"])
def test_ragged_and_sparse(case):
    """Padding rows (k = 25, 33), the spare record (points no multiple of four) and points
    with p = 0 and p < k (every 25th obs): the hit equals the fill equals no-reuse."""
    wl = dict(_ragged_cases())[case]
    if case == "spare":
        assert wl.points % 4 == 1
    inp = Inputs(wl)
    ref, = no_reuse(inp, [wl.var])
    if case == "sparse":
        assert 0 < ref[1]["solved"] < wl.points          # points with p = 0
        assert ref[1]["nobs_sum"] / ref[1]["solved"] < wl.k  # and with p < k
    r = Run(inp)
    try:
        fill = r.call(wl.var)
        is_miss(fill[2])
        nbat = fill[2]["batches_assembled"]
        hit = r.call(wl.var)
        is_hit(hit[2], nbat)
        same(fill[:2], ref)
        same(hit[:2], ref)
    finally:
        r.close()


def test_partial_budget(w):
    """14 MiB hold the records of two batches of 1024 points (2 x 1025 x 6880 B = 13.5 MiB)
    and not of three (20.2 MiB): the second call reuses exactly those two and assembles the
    other 42; the result equals no-reuse."""
    inp = Inputs(w)
    var2 = other_var(w, 9)
    ref1, ref2 = no_reuse(inp, [w.var, var2])
    r = Run(inp, reuse=14)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 44)
        assert 2 * 1025 * REC_BYTES <= info["bytes_held"] < 3 * 1025 * REC_BYTES
        same((out, cnt), ref1)
        for var, ref in ((w.var, ref1), (var2, ref2)):
            out, cnt, info = r.call(var)
            assert info["batches_reused"] == 2 and info["batches_assembled"] == 42, info
            same((out, cnt), ref)
    finally:
        r.close()


def test_host_slab(w):
    """A pageable host slab: the compare runs on the staged coordinates; fill, then hit, both
    equal to the device-slab analysis."""
    inp = Inputs(w)
    ref, = no_reuse(inp, [w.var])
    r = Run(inp, host=True)
    try:
        fill = r.call(w.var)
        is_miss(fill[2])
        hit = r.call(w.var)
        is_hit(hit[2], fill[2]["batches_assembled"])
        same(fill[:2], ref)
        same(hit[:2], ref)
        r.alt += np.float32(37.0)  # the caller's array rewritten in place: a miss
        is_miss(r.call(w.var)[2])
    finally:
        r.close()


@pytest.mark.parametrize("window", [256, 2500])
def test_info_window_rollover_on_hit(w, window):
    """Small info windows (one per batch at 256; two batches and a rollover mid-call at 2500):
    the hit restores the accepted counts window by window, and the counters and the analysis
    equal the default window's."""
    inp = Inputs(w)
    ref, = no_reuse(inp, [w.var])
    r = Run(inp, opts={"info_window": window})
    try:
        fill = r.call(w.var)
        is_miss(fill[2])
        hit = r.call(w.var)
        is_hit(hit[2], fill[2]["batches_assembled"])
        same(fill[:2], ref)
        same(hit[:2], ref)
    finally:
        r.close()


def test_budget_below_one_batch(w):
    """1 MiB holds no batch's records (7 MB each): the calls succeed, keep and reuse nothing
    and equal no-reuse."""
    inp = Inputs(w)
    ref, = no_reuse(inp, [w.var])
    r = Run(inp, reuse=1)
    try:
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 44)
            assert info["bytes_held"] == 0, info
            same((out, cnt), ref)
    finally:
        r.close()


def test_option_range():
    c = abi.Core(40, device=0)
    try:
        with pytest.raises(abi.CwblError, match="ARG"):
            c.set_option("record_reuse", -1)
        c.set_option("record_reuse", 0)
    finally:
        c.finalize()
