"""GPU tests of the step scalars kept beside the cached factor (CWBL_OPT_FACTOR_REUSE).

The fill stores what each step's dlarfg produced: scal at row j + 1 of the factor's column j,
beta and tau in an 80-word entry of their own per cached point (FactorAux).  A hit loads them
and runs no dlarfg.  The loaded bits are the fill's, so every comparison is exact, as in
test_gpu_factor_reuse.py: np.array_equal on the bit patterns and equal counters against the
analysis with record_reuse = 0.

The cases are the ones where a stored scalar differs in kind from a recomputed one, or where an
entry could be taken from the wrong place: reflectors that are exactly the identity (xx == 0:
beta = alpha, tau = 0, scal = 0), NaN records, the seams of the entry buffer (sub-batches, the
spare entry, a refill of another size), and what the cache reports as held.
"""
import numpy as np
import pytest

from cwbl import abi, synth

from reuse_harness import Inputs, Run, is_hit, is_miss, no_reuse, other_var, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL = {"max_batch": 256, "split40_batch": 128}
AUX_BYTES = 640  # FactorAux<40>: 80 fp64 words


def fill_then_hits(inp, variables, want, opts):
    """A fill on variables[0], then a hit on every variable: each equals `want`."""
    r = Run(inp, opts=opts)
    try:
        out, cnt, info = r.call(variables[0])
        is_miss(info)
        nbat = info["batches_assembled"]
        same((out, cnt), want[0])
        for var, ref in zip(variables, want):
            out, cnt, info = r.call(var)
            is_hit(info, nbat)
            same((out, cnt), ref)
    finally:
        r.close()


def test_exact_zero_reflectors():
    """Eight obs in all: every solved point has p < k - 2, A - inflat I has rank p, and the
    steps past it meet an exactly zero pivot column (dlarfg's xx == 0 branch: tau = 0,
    scal = 0, beta = alpha).  Those zeros are stored and loaded like any other value."""
    wl = synth.make("c2", nx=12, ny=12, nz=5, n_obs=8)
    inp = Inputs(wl)
    v2 = other_var(wl, 3)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    cnt = want[0][1]
    assert cnt["solved"] > 0
    assert 0 < cnt["nobs_sum"] / cnt["solved"] <= cnt["max_p"] < wl.k - 2, cnt
    fill_then_hits(inp, [wl.var, v2], want, SMALL)


def test_nan_records(monkeypatch):
    """weight_function = 1 (test_gpu_column_share.py's Gaspari-Cohn workload): the fp32 weights
    are NaN at some points, whose records, factors and step scalars are NaN.  The fill and the
    hits carry the same NaN bit patterns as the analysis without reuse."""
    core = abi.Core
    monkeypatch.setattr(abi, "Core", lambda *a, **kw: core(*a, weight_function=1, **kw))
    wl = synth.make("c2", nx=13, ny=11, nz=5, k=40, vclr=-1.0, hclr=6.0, n_obs=300)
    inp = Inputs(wl)
    v2 = other_var(wl, 3)
    want = no_reuse(inp, [wl.var, v2], opts=SMALL)
    nan = np.isnan(want[0][0]).any(axis=0)
    print(f"gaspari-cohn: {int(nan.sum())} NaN points of {wl.points}")
    assert 0 < nan.sum() < wl.points
    fill_then_hits(inp, [wl.var, v2], want, SMALL)


@pytest.mark.parametrize("sub", [37, 50])
def test_aux_seams(sub):
    """715 points (13 x 11 x 5, no multiple of four) in batches of 256 and sub-batches of 37 or
    50 points: every sub-batch's entries start where its records do, and the lanes past a
    launch read the spare entry.  Then hclr and ix_lim change (770 points): the refill needs a
    larger buffer; and back (715: the buffer keeps the other fill's entries past the end).
    Every call equals its own analysis without reuse, so no stale or neighbouring entry is
    ever used."""
    wl = synth.make("c2", nx=14, ny=11, nz=5, n_obs=120)
    a, b = Inputs(wl), Inputs(wl)
    a.ix_lim = 13
    b.tp.hclr = 10.0
    opts = {"max_batch": 256, "split40_batch": sub}
    v2 = other_var(wl, 5)
    want_a = no_reuse(a, [wl.var, v2], opts=opts)
    want_b = no_reuse(b, [wl.var, v2], opts=opts)
    assert want_a[0][1]["points"] == 715 and want_b[0][1]["points"] == 770
    assert want_a[0][1]["solved"] > 0 and want_b[0][1]["solved"] > 0
    r = Run(a, opts=opts)
    try:
        for cur, want in ((a, want_a), (b, want_b), (a, want_a)):
            r.sync(cur)
            out, cnt, info = r.call(wl.var)
            is_miss(info)
            nbat = info["batches_assembled"]
            same((out, cnt), want[0])
            for var, ref in ((v2, want[1]), (wl.var, want[0])):
                out, cnt, info = r.call(var)
                is_hit(info, nbat)
                same((out, cnt), ref)
    finally:
        r.close()


def test_accounting():
    """The budget bounds the records alone: 14 MiB keeps two batches of 1 025 records with
    factor_reuse on or off.  The entries of the step scalars lie outside it and are reported
    in bytes_held: 640 B per cached point and spare (2 050), with at most 1/16 of headroom;
    a refill with factor_reuse = 0 gives them back."""
    wl = synth.make("c2", scale=0.1)
    inp = Inputs(wl)
    held, reused = {}, {}
    for fr in (0, 1):
        r = Run(inp, reuse=14, opts={"factor_reuse": fr})
        try:
            _, _, info = r.call(wl.var)
            is_miss(info, 44)
            held[fr] = info["bytes_held"]
            _, _, info = r.call(wl.var)
            reused[fr] = info["batches_reused"]
            assert info["bytes_held"] == held[fr], info
            if fr == 1:
                r.c.set_option("factor_reuse", 0)
                _, _, info = r.call(wl.var)
                is_miss(info, 44)
                assert info["bytes_held"] == held[0], (info, held)
        finally:
            r.close()
    assert reused[0] == reused[1] == 2, reused
    aux = held[1] - held[0]
    floor = AUX_BYTES * (2 * 1024 + 2)  # cached points + cached batches (one spare each)
    print(f"bytes_held: records {held[0]}, with step scalars {held[1]} (+{aux}, floor {floor})")
    assert floor <= aux < 2 * floor, (held, floor)
