"""GPU tests of the cell-order numbering of the device-built search index
(CWBL_OPT_INDEX_ORDER = 1 under CWBL_OPT_INDEX = 1, cwbl_index_info, cwbl_index_slots).

Under order 1 a column's slot is its position in the cell-sorted order of its type's bins
instead of its obs index.  A point's neighbour list keeps its order under both numberings: the
same cells are visited, the order inside a cell is ascending obs index, and a truncated list
follows kdtree2's order; only the labels differ, and the column behind a label is the same
obs.  So every comparison with order 0 is exact: np.array_equal on the bit patterns and equal
counters.  Against index mode 0 the bar is that of test_gpu_index (equal counters, increments
within 1e-9 relative RMS), against the reference's output INCR_TOL.

The workloads are those of tests/test_gpu_index.py (CASES) and tests/gts_cases.py (720 points in
batches of 256, 256 and 208).
"""
import numpy as np
import pytest

import gts_cases as gc
from cwbl import abi
from helpers import increment_rel_rms
from reuse_harness import BATCH, is_hit, is_miss, same
from test_gpu_analyze_vars import bits, variables
from test_gpu_analyze_vars_big_mixed import nan_aware_equal
from test_gpu_gts_large_k import GtsInputs, GtsLib, GtsRun
from test_gpu_index import CASES, INCR_TOL, analyse, case_of, counts, fresh_core

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORDER1 = {"index": 1, "index_order": 1}
ORDER0 = {"index": 1}
_runs = {}


def all_slots(core):
    """{(family, type id): slot -> obs index table} of the types the last call used."""
    out = {}
    for family, ntypes in ((0, abi.NUM_GTS_TYPES), (1, abi.NUM_RADAR_TYPES)):
        for tid in range(1, ntypes + 1):
            try:
                out[(family, tid)] = core.index_slots(family, tid)
            except abi.CwblError as e:
                assert "ARG" in str(e), e
    return out


def run(name, **options):
    """test_gpu_index.analyse with the numbering beside it: (var, counts, prep info, index
    info, slot tables) of one analysis from a fresh library state; shared, never modified."""
    key = (name, tuple(sorted(options.items())))
    if key not in _runs:
        case = case_of(name)
        c = fresh_core(case, options)
        try:
            c.set_obs(case.obs())
            slab, var = case.slab()
            st = c.analyze_var(case.vp, slab)
            got = (var, counts(st), c.prep_info().as_dict(), c.index_info().as_dict(),
                   all_slots(c))
        finally:
            c.finalize()
        var.setflags(write=False)
        _runs[key] = got
    return _runs[key]


# ---- 1. every case against mode 1, order 0 -------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cell_order_equals_obs_order(name):
    case = case_of(name)
    v1, c1, p1, x1, s1 = run(name, **ORDER1)
    v0, c0, _ = analyse(name, index=1)
    vh, ch, _ = analyse(name, index=0)
    assert c1 == c0 == ch, (c1, c0, ch)
    assert c1[0] > 0
    np.testing.assert_array_equal(v1.view(np.uint32), v0.view(np.uint32))
    rel = increment_rel_rms(v1, vh, case.var_in)
    print(f"{name}: order 1 vs mode 0 rel rms {rel:.3e}; counts {c1}; prep {p1}; index {x1}")
    assert rel <= 1e-9, rel
    if case.var_out is not None:
        assert increment_rel_rms(v1, case.var_out, case.var_in) <= INCR_TOL
    assert x1["index_mode"] == 1 and x1["cell_order"] == 1
    assert x1["types"] == len(s1) > 0
    assert p1["bins_on_device"] == p1["bins_built"] == x1["types"]
    for key, slots in s1.items():  # a permutation of the type's obs
        np.testing.assert_array_equal(np.sort(slots), np.arange(len(slots)), err_msg=str(key))


# ---- 2. the numbering itself ---------------------------------------------------------------------
@pytest.mark.parametrize("div", [0, 3])
def test_radar_slots_are_the_bins_order(div):
    """c5's radar type: the slot table is cwbl_bin_index's `order` for the type's coordinates,
    localisation and the call's divisor (0: both take it from the obs density); the identity
    under order 0; the k-d tree's permutation in mode 0."""
    case = case_of("c5")
    w = case.w
    tp = case.vp.radar[w.radar_type - 1]
    key = (1, w.radar_type)
    n = w.obs_xyz.shape[0]
    slots = run("c5", bin_div=div, **ORDER1)[4]
    assert list(slots) == [key]
    c = abi.Core(8, device=0)
    try:
        grid, _, order = c.bin_index(w.obs_xyz, tp.hclr, tp.vclr, div)
    finally:
        c.finalize()
    assert order.dtype == slots[key].dtype == np.int32 and len(order) == n
    np.testing.assert_array_equal(slots[key], order)
    assert grid.nbx * grid.nby * grid.nbz > 1 and not np.array_equal(order, np.arange(n))
    _, _, _, x0, s0 = run("c5", bin_div=div, **ORDER0)
    assert x0["cell_order"] == 0 and x0["index_mode"] == 1
    np.testing.assert_array_equal(s0[key], np.arange(n, dtype=np.int32))
    _, _, _, xh, sh = run("c5", bin_div=div, index=0)
    assert xh["cell_order"] == 0 and xh["index_mode"] == 0
    np.testing.assert_array_equal(np.sort(sh[key]), np.arange(n))


def gts_call(case, opts, var=None, vp=None):
    """One cwbl_analyze_var of a gts_cases.Case on a fresh core: (analysis, counters, index
    info, slot tables)."""
    lib = GtsLib(case, opts)
    try:
        out, cnt = lib.one(case.var if var is None else var, case.vp if vp is None else vp)
        return out, cnt, lib.c.index_info().as_dict(), all_slots(lib.c)
    finally:
        lib.close()


def test_gts_slots_are_the_bins_order():
    """SYNOP (five variables, 2-D) and SOUND (four variables, its own vclr > 0 but searched in
    2-D under Q1_REPLICATE: the GTS family's last type is 2-D) of the gts_cases base case."""
    case = gc.make("base", 40)
    _, _, x1, s1 = gts_call(case, dict(ORDER1, bin_div=2))
    _, _, x0, s0 = gts_call(case, dict(ORDER0, bin_div=2))
    assert x1["cell_order"] == 1 and x1["types"] == 4 == len(s1)
    assert x0["cell_order"] == 0 and x0["types"] == 4 == len(s0)
    c = abi.Core(8, device=0)
    try:
        for tid in (abi.GTS_SYNOP, abi.GTS_SOUND):
            xyz = case.gts[tid][0]
            _, _, order = c.bin_index(xyz, case.vp.gts[tid - 1].hclr, -1.0, 2)
            np.testing.assert_array_equal(s1[(0, tid)], order)
            assert not np.array_equal(order, np.arange(len(order)))
            np.testing.assert_array_equal(s0[(0, tid)], np.arange(len(order), dtype=np.int32))
    finally:
        c.finalize()


# ---- 3. truncated lists: the composed ind --------------------------------------------------------
@pytest.mark.parametrize("batch", [0, 256])
def test_truncated_lists_use_the_composed_tree(batch):
    name = "driver_mixed.npz"
    opts = {"max_batch": batch} if batch else {}
    v1, c1, p1, x1, _ = run(name, **dict(ORDER1, **opts))
    v0, c0, p0 = analyse(name, index=1, **opts)
    assert c1[2] > 0 and p1["flagged_batches"] > 0 and p1["trees_built"] > 0
    assert x1["trees_composed"] > 0 and x1["trees_composed"] <= p1["trees_built"]
    assert p1["flagged_batches"] == p0["flagged_batches"]
    assert c1 == c0
    np.testing.assert_array_equal(v1.view(np.uint32), v0.view(np.uint32))
    assert run(name, **dict(ORDER0, **opts))[3]["trees_composed"] == 0


# ---- 4. the tree walk for every point ------------------------------------------------------------
@pytest.mark.parametrize("name", ["driver_mixed.npz", "driver_c1.npz"])
def test_tree_walk_is_bit_identical_in_cell_order(name):
    v1, c1, p1, x1, _ = run(name, search=1, **ORDER1)
    v0, c0, _ = analyse(name, index=0, search=1)
    assert c1 == c0
    np.testing.assert_array_equal(v1.view(np.uint32), v0.view(np.uint32))
    assert x1["cell_order"] == 1 and x1["trees_composed"] == p1["trees_built"] == x1["types"]


# ---- 5. every stager -----------------------------------------------------------------------------
STAGERS = [(v, k) for k in (40, 64, 96, 128) for v in ("base", "q1_undef", "truncated")]


@pytest.mark.parametrize("variant,k", STAGERS, ids=[f"{v}-{k}" for v, k in STAGERS])
def test_gts_workload_on_every_path(variant, k):
    """k = 40: the record path; 64: stage_columns_pair; 96 and 128: stage_columns_pipe behind
    the hand-off kernels.  base: multi-variable types and rejected columns; q1_undef: the Q1
    undefined case; truncated: max_lz_pts = 6 for every type."""
    case = gc.make(variant, k)
    out1, cnt1, x1, _ = gts_call(case, ORDER1)
    out0, cnt0, x0, _ = gts_call(case, ORDER0)
    assert x1["cell_order"] == 1 and x0["cell_order"] == 0 and x1["types"] == x0["types"] > 0
    assert cnt1 == cnt0, (cnt1, cnt0)
    assert cnt1["solved"] > 0 and cnt1["nonconverged"] == 0
    assert nan_aware_equal(out1, out0)
    if variant == "truncated":
        assert cnt1["lz_truncated"] > 0 and x1["trees_composed"] > 0
    if variant == "q1_undef":
        assert cnt1["q1_undefined"] == case.points


def test_one_kernel_big_path():
    """big_path = 0: stage_columns with 256 threads."""
    case = gc.make("base", 96)
    out1, cnt1, _, _ = gts_call(case, dict(ORDER1, big_path=0))
    out0, cnt0, _, _ = gts_call(case, dict(ORDER0, big_path=0))
    assert cnt1 == cnt0 and cnt1["solved"] > 0
    assert nan_aware_equal(out1, out0)


def test_group_call_of_two_variables():
    case = gc.make("base", 64)
    vars_ = variables(case, 2)
    got = []
    for opts in (ORDER1, ORDER0):
        lib = GtsLib(case, opts)
        try:
            got.append(lib.group(vars_, [case.vp] * 2) + (lib.c.index_info().as_dict(),))
        finally:
            lib.close()
    (outs1, cnt1, x1), (outs0, cnt0, x0) = got
    assert x1["cell_order"] == 1 and x0["cell_order"] == 0
    assert cnt1 == cnt0 and cnt1["solved"] > 0
    for a, b in zip(outs1, outs0):
        assert nan_aware_equal(a, b)
    assert not nan_aware_equal(outs1[0], outs1[1])


def test_column_shared_call_on_the_2d_types():
    case = gc.make("flat", 96)
    got = []
    for opts in (ORDER1, ORDER0):
        lib = GtsLib(case, dict(opts, column_share=1))
        try:
            got.append(lib.one(case.var, case.vp) + (lib.c.index_info().as_dict(),
                                                     lib.c.column_info().as_dict()))
        finally:
            lib.close()
    (out1, cnt1, x1, ci1), (out0, cnt0, x0, ci0) = got
    assert ci1["shared"] == 1 and ci0["shared"] == 1
    assert x1["cell_order"] == 1 and x0["cell_order"] == 0
    assert cnt1 == cnt0 and cnt1["solved"] > 0
    assert np.array_equal(bits(out1), bits(out0))


def test_factor_cache_fill_and_hit():
    """k = 40 with the record cache on (it keeps factors): a fill and a hit with another
    variable under each numbering; what is cached does not depend on the numbering."""
    case = gc.make("base", 40)
    vars_ = variables(case, 2)
    core = dict(weight_function=case.weight_function, q1_mode=case.q1_mode)
    got = []
    for opts in (ORDER1, ORDER0):
        r = GtsRun(GtsInputs(case), reuse=256, opts=dict(BATCH, **opts), base={}, **core)
        try:
            fill = r.call(vars_[0])
            x = r.c.index_info().as_dict()
            hit = r.call(vars_[1])
            xh = r.c.index_info().as_dict()
        finally:
            r.close()
        is_miss(fill[2], 3, several=False)
        is_hit(hit[2], 3)
        assert xh["types"] == 0  # a full hit plans no index
        got.append((fill, hit, x))
    assert got[0][2]["cell_order"] == 1 and got[1][2]["cell_order"] == 0
    same(got[0][0], got[1][0])
    same(got[0][1], got[1][1])
    assert got[0][0][1]["solved"] > 0


# ---- 6. a changed divisor on a live core ---------------------------------------------------------
def test_changed_divisor_renumbers():
    name = "driver_mixed.npz"
    case = case_of(name)
    want, cw, _, xw, sw = run(name, bin_div=3, **ORDER1)
    c = fresh_core(case, dict(ORDER1, bin_div=0))
    try:
        c.set_obs(case.obs())
        slab, va = case.slab()
        sta = c.analyze_var(case.vp, slab)
        pa, xa, sa = c.prep_info().as_dict(), c.index_info().as_dict(), all_slots(c)
        c.set_option("bin_div", 3)
        slab, vb = case.slab()
        stb = c.analyze_var(case.vp, slab)
        pb, xb, sb = c.prep_info().as_dict(), c.index_info().as_dict(), all_slots(c)
    finally:
        c.finalize()
    assert pa["trees_built"] > 0 and xa["trees_composed"] > 0
    assert counts(stb) == cw == counts(sta)
    np.testing.assert_array_equal(vb.view(np.uint32), want.view(np.uint32))
    assert pb["bins_built"] == pb["bins_on_device"] == pa["bins_built"] > 0
    assert pb["trees_built"] == 0
    # the trees that were up are composed anew on the new numbering
    assert xb["cell_order"] == 1 and xb["trees_composed"] == xa["trees_composed"]
    assert sorted(sb) == sorted(sa) == sorted(sw)
    for key in sb:
        np.testing.assert_array_equal(sb[key], sw[key], err_msg=str(key))
    assert any(not np.array_equal(sb[key], sa[key]) for key in sb)
    np.testing.assert_array_equal(va.view(np.uint32), run(name, **ORDER1)[0].view(np.uint32))


# ---- 7. a device-resident obs set ----------------------------------------------------------------
def test_device_resident_obs_set():
    name = "driver_mixed.npz"
    case = case_of(name)
    d = case.driver
    v1, c1, _, _, s1 = run(name, **ORDER1)
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    c = fresh_core(case, ORDER1)
    try:
        c.set_obs(d.obs_set(memory=abi.MEM_DEVICE, to_device=to_dev))
        x, y, alt = (to_dev(np.asarray(a, np.float32)) for a in (d.x, d.y, d.alt))
        var = to_dev(np.asarray(d.var_in, np.float32).copy())
        torch.cuda.synchronize()
        slab = abi.make_slab(x, y, alt, var, d.ix_lim, d.iy_lim, memory=abi.MEM_DEVICE)
        st = c.analyze_var(case.vp, slab)
        got = var.cpu().numpy()
        info, slots = c.index_info().as_dict(), all_slots(c)
    finally:
        c.finalize()
    assert counts(st) == c1 and info["cell_order"] == 1
    np.testing.assert_array_equal(got.view(np.uint32), v1.view(np.uint32))
    assert sorted(slots) == sorted(s1)
    for key in slots:
        np.testing.assert_array_equal(slots[key], s1[key])


# ---- 8. ignored in mode 0; range, default and state ----------------------------------------------
def test_ignored_in_mode_0_and_option_range():
    name = "driver_c1.npz"
    case = case_of(name)
    v, cnt, p, x, s = run(name, index=0, index_order=1)
    v0, c0, _ = analyse(name, index=0)
    assert cnt == c0 and x["cell_order"] == 0 and x["index_mode"] == 0 and x["trees_composed"] == 0
    assert p["bins_on_device"] == 0
    np.testing.assert_array_equal(v.view(np.uint32), v0.view(np.uint32))
    c = fresh_core(case, ORDER1)
    try:
        with pytest.raises(abi.CwblError, match="ARG"):
            c.set_option("index_order", 2)
        with pytest.raises(abi.CwblError, match="ARG"):
            c.set_option("index_order", -1)
        with pytest.raises(abi.CwblError, match="STATE"):  # no call yet
            c.index_slots(0, abi.GTS_SYNOP)
        assert c.index_info().as_dict() == dict(index_mode=0, cell_order=0, types=0,
                                                trees_composed=0)
    finally:
        c.finalize()
    c = fresh_core(case, {"index": 1})  # cwbl_init resets the option: obs order again
    try:
        c.set_obs(case.obs())
        slab, var = case.slab()
        c.analyze_var(case.vp, slab)
        assert c.index_info().cell_order == 0
        with pytest.raises(abi.CwblError, match="ARG"):  # a type the call did not use
            c.index_slots(1, abi.RADAR_KDP)
    finally:
        c.finalize()
