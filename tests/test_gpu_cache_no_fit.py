"""GPU tests of the one corner where the record cache (CWBL_OPT_RECORD_REUSE) and the column
cache (CWBL_OPT_COLUMN_REUSE) answer differently: a fill of which no leading batch fits the
budget.  The record cache keeps the buffers of an earlier fill for the next one; the column cache
holds nothing.  Either way the call is a miss that equals the call with the cache off, bit for
bit.

Two ways there.  The budget shrinks below one batch's need: setting either option releases its
cache, so nothing is held afterwards in both.  Or the budget stays and the plan grows beyond it
(max_batch = 1024 makes one batch of the whole workload; the new generation makes the key
differ): here the two differ.

Workloads: reuse_harness.small(32), 720 points in batches of 256, 256 and 208, for the record
cache; test_gpu_column_reuse's 29 x 23 = 667 columns in batches of 256, 256 and 155 at k = 50 for
the column cache.  A batch of nb entries needs nb + 1 (the spare one).
"""
import pytest

from cwbl import abi
from reuse_harness import BATCH, Inputs, Run, is_hit, is_miss, no_reuse, same, small, small_refs
from test_gpu_column_reuse import BUDGET, COLUMN_BYTES, SEARCH, Seq, is_fill, kpc, reuse_opts, yard
from test_gpu_column_reuse import same as same_res

pytestmark = pytest.mark.gpu

MIB = 1 << 20
K_RECORD, K_COLUMN = 32, 50
POINTS, COLS = 720, 667
GRID = (29, 23)
WHOLE = {"max_batch": 1024}  # one batch of the whole workload


# ---- the record cache ----------------------------------------------------------------------------
def record_bytes():
    return COLUMN_BYTES[kpc(K_RECORD)]  # AsmRecord<40>, the budget's unit in both forms of k <= 40


def test_record_cache_budget_shrinks_below_a_batch():
    w = small(K_RECORD)
    assert 257 * record_bytes() > MIB
    want = small_refs(K_RECORD)[0]
    r = Run(Inputs(w), reuse=BUDGET, opts=BATCH)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        assert info["bytes_held"] >= (POINTS + 3) * record_bytes(), info
        is_hit(r.call(w.var)[2], 3)
        r.c.set_option("record_reuse", 1)
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 3)
            assert info["bytes_held"] == 0, info
            same((out, cnt), want)
    finally:
        r.close()


def test_record_cache_plan_grows_beyond_the_budget():
    """... and the buffers of the earlier fill stay: the next fill that fits takes them as they
    are, and hits."""
    w = small(K_RECORD)
    per, budget = record_bytes(), 2
    assert 257 * per <= budget * MIB < 2 * 257 * per and (POINTS + 1) * per > budget * MIB
    want = small_refs(K_RECORD)[0]
    want_whole, = no_reuse(Inputs(w), [w.var], opts=WHOLE)
    r = Run(Inputs(w), reuse=budget, opts=BATCH)
    try:
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        held = info["bytes_held"]
        assert 257 * per <= held, info
        info = r.call(w.var)[2]
        assert info["batches_reused"] == 1 and info["batches_assembled"] == 2, info
        r.c.set_option("max_batch", WHOLE["max_batch"])
        for _ in range(2):
            out, cnt, info = r.call(w.var)
            is_miss(info, 1, several=False)
            assert info["bytes_held"] == held, (info, held)
            same((out, cnt), want_whole)
        r.c.set_option("max_batch", BATCH["max_batch"])
        out, cnt, info = r.call(w.var)
        is_miss(info, 3)
        assert info["bytes_held"] == held, (info, held)
        same((out, cnt), want)
        out, cnt, info = r.call(w.var)
        assert info["batches_reused"] == 1 and info["batches_assembled"] == 2, info
        assert info["bytes_held"] == held, (info, held)
        same((out, cnt), want)
    finally:
        r.close()


# ---- the column cache ----------------------------------------------------------------------------
def column_opts(budget, max_batch=256):
    return reuse_opts(K_COLUMN, (("max_batch", max_batch),), budget)


def column_yard(nz, max_batch=256):
    base = tuple((n, v) for n, v in column_opts(0, max_batch) if n != "column_reuse")
    return yard(K_COLUMN, "dense", nz, "", base, *GRID)


def holds_nothing(r):
    assert r.reuse["bytes_held"] == 0 and r.reuse["form"] == abi.COLUMN_FORM_NONE, r.reuse
    assert r.reuse["columns_filled"] == r.reuse["columns_reused"] == 0, r.reuse
    assert r.reuse["batches_reused"] == 0, r.reuse
    assert r.info["shared"] == 1 and r.info["columns"] == COLS, r.info


def test_column_cache_budget_shrinks_below_a_batch():
    assert 257 * COLUMN_BYTES[kpc(K_COLUMN)] > MIB
    s = Seq(K_COLUMN, "dense", column_opts(BUDGET), *GRID)
    try:
        a = s.call(3)
        s.lib.c.set_option("column_reuse", 1)
        got = [s.call(3), s.call(3)]
    finally:
        s.close()
    is_fill(a, K_COLUMN, 3, COLS)
    for r in got:
        holds_nothing(r)
        same_res(r, column_yard(3))


def test_column_cache_plan_grows_beyond_the_budget():
    """... and everything is released; the next fill that fits allocates afresh, and hits."""
    per, budget = COLUMN_BYTES[kpc(K_COLUMN)], 4
    assert 257 * per <= budget * MIB < 2 * 257 * per and (COLS + 1) * per > budget * MIB
    s = Seq(K_COLUMN, "dense", column_opts(budget), *GRID)
    try:
        a, b = s.call(3), s.call(1)
        s.lib.c.set_option("max_batch", WHOLE["max_batch"])
        got = [s.call(3), s.call(3)]
        s.lib.c.set_option("max_batch", 256)
        c, d = s.call(3), s.call(1)
    finally:
        s.close()
    for fill, hit in ((a, b), (c, d)):
        assert fill.reuse["columns_filled"] == 256 and fill.reuse["batches_reused"] == 0, fill.reuse
        assert fill.reuse["bytes_held"] >= 257 * per, fill.reuse
        assert hit.reuse["columns_reused"] == 256 and hit.reuse["batches_reused"] == 1, hit.reuse
        assert hit.reuse["bytes_held"] == fill.reuse["bytes_held"], (hit.reuse, fill.reuse)
        same_res(fill, column_yard(3))
        same_res(hit, column_yard(1))
    for r in got:
        holds_nothing(r)
        assert r.kt[SEARCH]["launches"] == 1 and r.kt[SEARCH]["points"] == COLS, r.kt
        same_res(r, column_yard(3, WHOLE["max_batch"]))
