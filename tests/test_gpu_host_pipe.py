"""GPU tests of CWBL_OPT_HOST_PIPE: the host-memory slabs of group calls, column-shared calls and
calls with tune_q = 1 piped batch by batch (S.h2d up, S.d2h back, tune_q_kernel over each
batch behind its solve) where they otherwise move whole around the batches.

The yardstick of every case is the same call on device slabs with the option 0: np.array_equal
on the bit patterns of every variable, and equal counters.  cwbl_transfer_info says which way
the host call's var travelled; the byte counts it reports must be exactly the slabs' sizes.

Workloads: synth c2 on 12 x 12 x 5 = 720 points in search batches of 256 (256, 256, 208: an
upload, a solve and a copy back in flight together, a ragged last batch, batch boundaries
inside a level plane); the column-shared cases on 32 x 24 = 768 columns (a multiple of 4, so
the comparison with the per-point call's grouping is exact) of 5 levels, three column batches.
"""
import collections
import copy
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from test_gpu_analyze_vars import Lib, bits, counters, other_var

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NBAT = 3
TUNE = "tune_q_kernel"
Res = collections.namedtuple("Res", "outs cnt ti reuse kt col")


def opts_of(k, **more):
    o = {"max_batch": 256}
    if k > 64:
        o["big_batch"] = 128  # two hand-off sub-batches per search batch
    o.update(more)
    return o


@functools.lru_cache(maxsize=None)
def small(k):
    """12 x 12 x 5 points, 120 obs: 720 points, batches of 256, 256 and 208."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)


@functools.lru_cache(maxsize=None)
def sparse(k):
    """The same grid with 30 obs of a short radius: more than half of the points have no obs
    in reach (p = 0; 337 of 720 are solved), five of them in the DRY row."""
    return synth.make("c2", nx=12, ny=12, nz=5, n_obs=30, k=k, hclr=0.8)


@functools.lru_cache(maxsize=None)
def columns(k):
    """32 x 24 columns of 5 levels with 2-D localisation: a column-shared call's workload."""
    return synth.make("c2", nx=32, ny=24, nz=5, k=k, vclr=-1.0, hclr=0.8, n_obs=60)


DRY = (3, 7)  # level and row of the points with no positive member


def q_vars(w, n):
    return _q_vars(w.var.shape, n)


@functools.lru_cache(maxsize=None)
def _q_vars(shape, n):
    """n moist-variable look-alikes: N(1, 1) members, so about one in six is negative, and a
    row of points whose members are negative or zero (letkf_tune_q's x/0: Q3's NaN on the
    zeros)."""
    out = []
    for i in range(n):
        rng = np.random.default_rng(300 + i)
        v = rng.standard_normal(shape, dtype=np.float32) + np.float32(1.0)
        row = v[(slice(None),) + DRY]  # (k, nx), a view
        row[0::2] = -np.abs(row[0::2]) - 1.0
        row[1::2] = 0.0
        out.append(v)
    return tuple(out)


def plain_vars(w, n):
    return tuple([w.var] + [other_var(w, 100 + i) for i in range(1, n)])


def tuned(vp, flag=1):
    vp = copy.deepcopy(vp)
    vp.tune_q = flag
    return vp


def call(w, vars_, vps, opts, mem, single=False, ix_lim=None, ncalls=1, between=None):
    """`ncalls` analyses of copies of vars_ (cwbl_analyze_var when single, else
    cwbl_analyze_vars) on one library state; mem: "device", "pageable" numpy slabs or "pinned"
    (torch pin_memory) ones.  between(core, i) runs before call i > 0.  -> [Res]"""
    lib = Lib(w, opts, host=mem != "device")
    res = []
    try:
        for i in range(ncalls):
            if i and between:
                between(lib.c, i)
            keep = None
            if mem == "pinned":
                keep = [torch.empty(v.shape, dtype=torch.float32).pin_memory() for v in vars_]
                bufs = [t.numpy() for t in keep]
                for b, v in zip(bufs, vars_):
                    b[...] = v
            else:
                bufs = lib.buffers(vars_)
            lib.c.set_kernel_timing(True)
            slabs = [lib.slab(b, ix_lim) for b in bufs]
            st = lib.c.analyze_var(vps[0], slabs[0]) if single else lib.c.analyze_vars(vps, slabs)
            outs = [np.array(lib.fetch(b), copy=True) for b in bufs]
            res.append(Res(outs, counters(st), lib.c.transfer_info().as_dict(),
                           lib.c.reuse_info().as_dict(), lib.c.kernel_times(),
                           lib.c.column_info().as_dict()))
            del keep
    finally:
        lib.close()
    return res


@functools.lru_cache(maxsize=None)
def reference(wname, k, vkind, nvar, flags, opts, single=False, ix_lim=None, ncalls=1):
    """The yardstick: the call on device slabs with host_pipe = 0.  Shared, never modified."""
    w = {"small": small, "sparse": sparse, "columns": columns}[wname](k)
    vars_ = (q_vars if vkind == "q" else plain_vars)(w, nvar)
    vps = [tuned(w.vp, f) for f in flags]
    o = dict(opts)
    o["host_pipe"] = 0
    res = call(w, vars_, vps, o, "device", single, ix_lim, ncalls)
    for r in res:
        assert r.ti == dict.fromkeys(r.ti, 0) | {"tune_q_launches": sum(flags)}, r.ti
        assert r.cnt["solved"] > 0
    return w, vars_, vps, res


def same(got, ref):
    assert got.cnt == ref.cnt, (got.cnt, ref.cnt)
    assert len(got.outs) == len(ref.outs)
    for i, (a, b) in enumerate(zip(got.outs, ref.outs)):
        assert np.array_equal(bits(a), bits(b)), i


def nbytes(vars_):
    return sum(v.nbytes for v in vars_)


def is_piped(ti, vars_, registered, bounce=0, tune_launches=0):
    assert ti == {"host": 1, "piped": 1, "piped_back": 1, "registered": registered,
                  "bounce": bounce, "reason": abi.TRANSFER_PIPED,
                  "tune_q_launches": tune_launches, "bytes_piped_up": nbytes(vars_),
                  "bytes_piped_down": nbytes(vars_), "bytes_whole_up": 0,
                  "bytes_whole_down": 0}, ti


def is_whole(ti, vars_, reason):
    assert ti["host"] == 1 and ti["piped"] == 0 and ti["piped_back"] == 0, ti
    assert ti["registered"] == 0 and ti["bounce"] == 0 and ti["reason"] == reason, ti
    assert ti["bytes_piped_up"] == 0 and ti["bytes_piped_down"] == 0, ti
    assert ti["bytes_whole_up"] == nbytes(vars_) == ti["bytes_whole_down"], ti


def frozen(o):
    return tuple(sorted(o.items()))


# ---- group calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("nvar", [3, 8])
@pytest.mark.parametrize("k", [40, 16, 64, 96])
def test_group_is_piped(k, nvar, mem):
    """Record path (40), one-wavefront path (16, 64), hand-off path with two sub-batches (96)."""
    o = opts_of(k)
    w, vars_, vps, (ref,) = reference("small", k, "plain", nvar, (0,) * nvar, frozen(o))
    assert ref.reuse["batches_assembled"] == NBAT
    assert not np.array_equal(bits(ref.outs[0]), bits(vars_[0]))  # the call analysed something
    got, = call(w, vars_, vps, dict(o, host_pipe=1), mem)
    same(got, ref)
    assert got.reuse["batches_assembled"] == NBAT
    is_piped(got.ti, vars_, registered=nvar if mem == "pageable" else 0)
    # the same kernels ran, over the same points
    assert {n: (t["launches"], t["points"]) for n, t in got.kt.items()} == \
           {n: (t["launches"], t["points"]) for n, t in ref.kt.items()}


@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("k", [40, 64, 96])
def test_group_with_mixed_tune_q(k, mem):
    """tune_q on three of four variables, sparse obs: the points the solve skips (p = 0) are
    tuned as well, per batch, and the variable without the flag keeps its negative members."""
    flags = (1, 0, 1, 1)
    o = opts_of(k)
    w, vars_, vps, (ref,) = reference("sparse", k, "q", 4, flags, frozen(o))
    assert 0 < ref.cnt["solved"] < ref.cnt["points"] // 2  # most points have p = 0
    assert ref.kt[TUNE]["launches"] == 3 and ref.kt[TUNE]["points"] == 3 * 720
    got, = call(w, vars_, vps, dict(o, host_pipe=1), mem)
    same(got, ref)
    is_piped(got.ti, vars_, registered=4 if mem == "pageable" else 0, tune_launches=NBAT * 3)
    assert got.kt[TUNE]["launches"] == NBAT * 3 and got.kt[TUNE]["points"] == 3 * 720, got.kt
    # the points the solve skipped: where the variable without the flag kept every bit
    plain = flags.index(0)
    skipped = (bits(got.outs[plain]) == bits(vars_[plain])).all(axis=0)  # (nz, ny, nx)
    assert skipped.sum() == ref.cnt["points"] - ref.cnt["solved"]
    row = np.zeros_like(skipped)
    row[DRY] = True
    dry = row & skipped
    assert dry.any()
    for out, var, f in zip(got.outs, vars_, flags):
        neg = (var < 0) & skipped
        assert neg.sum() > skipped.sum()  # more than one negative member per point
        if f:  # `where (var < 0) 0` there too, and x/0 times the dry points' zeros
            assert not out[neg].any()
            assert np.isnan(out[1::2][:, dry]).all()
            assert not np.isnan(out[:, ~row]).any()
        else:
            assert np.array_equal(bits(out[neg]), bits(var[neg]))


@pytest.mark.parametrize("k", [40, 64])
def test_small_info_window(k):
    """info_window = 256: a window closes at every batch of the piped group call."""
    o = opts_of(k, info_window=256)
    w, vars_, vps, (ref,) = reference("small", k, "plain", 3, (0, 0, 0), frozen(o))
    got, = call(w, vars_, vps, dict(o, host_pipe=1), "pageable")
    same(got, ref)
    is_piped(got.ti, vars_, registered=3)
    # ... and the counters do not depend on the window
    assert ref.cnt == reference("small", k, "plain", 3, (0, 0, 0), frozen(opts_of(k)))[3][0].cnt


# ---- single calls with tune_q ------------------------------------------------------------------
HOSTS = {"registered": ("pageable", {}, dict(registered=1)),
         "pinned": ("pinned", {}, dict(registered=0)),
         "bounce": ("pageable", {"pageable": 1}, dict(registered=0, bounce=1))}


@pytest.mark.parametrize("host", sorted(HOSTS))
@pytest.mark.parametrize("k", [40, 64, 96])
def test_single_tune_q_comes_back_piped(k, host):
    mem, more, want = HOSTS[host]
    o = opts_of(k)
    w, vars_, vps, (ref,) = reference("sparse", k, "q", 1, (1,), frozen(o), single=True)
    assert 0 < ref.cnt["solved"] < ref.cnt["points"]
    got, = call(w, vars_, vps, dict(o, host_pipe=1, **more), mem, single=True)
    same(got, ref)
    is_piped(got.ti, vars_, tune_launches=NBAT, **want)
    assert got.kt[TUNE]["launches"] == NBAT and got.kt[TUNE]["points"] == 720, got.kt
    assert np.isnan(got.outs[0]).any()  # a dry point that the solve skipped


def test_single_tune_q_off_comes_back_whole():
    """Option 0: piped up, tuned once after the last batch, back whole."""
    o = opts_of(40)
    w, vars_, vps, (ref,) = reference("sparse", 40, "q", 1, (1,), frozen(o), single=True)
    got, = call(w, vars_, vps, dict(o, host_pipe=0), "pageable", single=True)
    same(got, ref)
    ti = got.ti
    assert ti["piped"] == 1 and ti["piped_back"] == 0 and ti["registered"] == 1, ti
    assert ti["reason"] == abi.TRANSFER_REASON_OFF and ti["tune_q_launches"] == 1, ti
    assert ti["bytes_piped_up"] == nbytes(vars_) == ti["bytes_whole_down"], ti
    assert ti["bytes_piped_down"] == 0 and ti["bytes_whole_up"] == 0, ti


@pytest.mark.parametrize("host", sorted(HOSTS))
@pytest.mark.parametrize("k,more", [(40, {}), (64, {"wave_reuse": 1})])
def test_cache_fill_then_hit(k, more, host):
    """A fill and a hit of the record cache (k = 40) and of the factor cache (k = 64), both
    with tune_q per batch."""
    mem, hmore, want = HOSTS[host]
    o = opts_of(k, record_reuse=64, **more)
    w, vars_, vps, refs = reference("sparse", k, "q", 1, (1,), frozen(o), single=True, ncalls=2)
    assert refs[0].reuse["batches_reused"] == 0 and refs[1].reuse["batches_reused"] == NBAT
    gots = call(w, vars_, vps, dict(o, host_pipe=1, **hmore), mem, single=True, ncalls=2)
    for got, ref in zip(gots, refs):
        same(got, ref)
        assert got.reuse["batches_reused"] == ref.reuse["batches_reused"], got.reuse
        is_piped(got.ti, vars_, tune_launches=NBAT, **want)


def test_partial_budget():
    """2 MiB hold the first batch's 257 records and not the second's: the next call solves one
    batch from the cache and two afresh, every one tuned and returned per batch."""
    o = opts_of(40, record_reuse=2)
    w, vars_, vps, refs = reference("sparse", 40, "q", 1, (1,), frozen(o), single=True, ncalls=2)
    assert refs[1].reuse["batches_reused"] == 1 and refs[1].reuse["batches_assembled"] == 2
    gots = call(w, vars_, vps, dict(o, host_pipe=1), "pageable", single=True, ncalls=2)
    for got, ref in zip(gots, refs):
        same(got, ref)
        assert got.reuse["batches_reused"] == ref.reuse["batches_reused"], got.reuse
        is_piped(got.ti, vars_, registered=1, tune_launches=NBAT)


def test_toggling_the_option_keeps_the_cache():
    """host_pipe set between a fill and the next calls: a hit is reported each time."""
    o = opts_of(40, record_reuse=64)
    w, vars_, vps, refs = reference("sparse", 40, "q", 1, (1,), frozen(o), single=True, ncalls=3)

    def toggle(core, i):
        core.set_option("host_pipe", i % 2)

    gots = call(w, vars_, vps, dict(o, host_pipe=0), "pageable", single=True, ncalls=3,
                between=toggle)
    for got, ref in zip(gots, refs):
        same(got, ref)
    assert [g.reuse["batches_reused"] for g in gots] == [0, NBAT, NBAT]
    assert [g.ti["piped_back"] for g in gots] == [0, 1, 0]
    assert [g.ti["tune_q_launches"] for g in gots] == [1, NBAT, 1]


# ---- column-shared calls -----------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("tune", [0, 1])
@pytest.mark.parametrize("share", [1, 2])
@pytest.mark.parametrize("k", [40, 64])
def test_column_shared_is_piped(k, share, tune, mem):
    o = opts_of(k, column_share=share)
    w, vars_, vps, (ref,) = reference("columns", k, "q" if tune else "plain", 1, (tune,),
                                      frozen(o), single=True)
    assert ref.col["shared"] == 1 and ref.col["columns"] == 768 and ref.col["levels"] == 5
    assert ref.reuse["batches_assembled"] == NBAT  # column batches
    assert 0 < ref.cnt["solved"]
    got, = call(w, vars_, vps, dict(o, host_pipe=1), mem, single=True)
    same(got, ref)
    assert got.col == ref.col
    # (one 2-D launch per column batch covers its columns at every level)
    is_piped(got.ti, vars_, registered=1 if mem == "pageable" else 0, tune_launches=NBAT * tune)
    if tune:
        assert got.kt[TUNE]["launches"] == NBAT and got.kt[TUNE]["points"] == 768 * 5, got.kt
    else:
        assert TUNE not in got.kt


# ---- fall-backs --------------------------------------------------------------------------------
def test_option_off_moves_a_group_whole():
    o = opts_of(40)
    w, vars_, vps, (ref,) = reference("small", 40, "plain", 3, (0, 0, 0), frozen(o))
    got, = call(w, vars_, vps, dict(o, host_pipe=0), "pageable")
    same(got, ref)
    is_whole(got.ti, vars_, abi.TRANSFER_REASON_OFF)
    # ... which is the default
    got, = call(w, vars_, vps, o, "pageable")
    same(got, ref)
    is_whole(got.ti, vars_, abi.TRANSFER_REASON_OFF)


def test_option_off_moves_a_column_shared_call_whole():
    o = opts_of(40, column_share=1)
    w, vars_, vps, (ref,) = reference("columns", 40, "q", 1, (1,), frozen(o), single=True)
    got, = call(w, vars_, vps, dict(o, host_pipe=0), "pageable", single=True)
    same(got, ref)
    assert got.col["shared"] == 1
    is_whole(got.ti, vars_, abi.TRANSFER_REASON_OFF)
    assert got.ti["tune_q_launches"] == 1


@pytest.mark.parametrize("k", [40, 64])
def test_staggered_group_moves_whole(k):
    o = opts_of(k)
    nx = small(k).nx
    w, vars_, vps, (ref,) = reference("small", k, "q", 2, (1, 0), frozen(o), ix_lim=nx - 1)
    assert ref.cnt["points"] == (nx - 1) * w.ny * w.nz
    got, = call(w, vars_, vps, dict(o, host_pipe=1), "pageable", ix_lim=nx - 1)
    same(got, ref)
    is_whole(got.ti, vars_, abi.TRANSFER_REASON_REGION)
    assert got.ti["tune_q_launches"] == 1
    for out, var in zip(got.outs, vars_):  # the last column is not analysed, nor tuned
        assert np.array_equal(bits(out[..., -1]), bits(var[..., -1]))


def test_bounce_slots_with_a_group_move_whole():
    o = opts_of(40)
    w, vars_, vps, (ref,) = reference("small", 40, "plain", 3, (0, 0, 0), frozen(o))
    got, = call(w, vars_, vps, dict(o, host_pipe=1, pageable=1), "pageable")
    same(got, ref)
    is_whole(got.ti, vars_, abi.TRANSFER_REASON_BOUNCE)
    # page-locked slabs need no slot: piped whatever CWBL_OPT_PAGEABLE says
    got, = call(w, vars_, vps, dict(o, host_pipe=1, pageable=1), "pinned")
    same(got, ref)
    is_piped(got.ti, vars_, registered=0)


def test_option_range():
    c = abi.Core(8, device=0)
    try:
        for bad in (-1, 2):
            with pytest.raises(abi.CwblError, match="out of range"):
                c.set_option("host_pipe", bad)
        c.set_option("host_pipe", 1)
        c.set_option("host_pipe", 0)
    finally:
        c.finalize()
