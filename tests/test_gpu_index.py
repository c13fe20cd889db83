"""GPU tests of the device-built search index (CWBL_OPT_INDEX = 1, cwbl_bin_index,
cwbl_prep_info).

Bins: cwbl_bin_index against a numpy restatement.  The cell ids are recomputed in fp32 from the
returned grid (the arithmetic of build_bins: floor((v - origin) * binv) clamped to the grid, a
point with a non-finite coordinate in cell 0); the expected arrays are the stable sort of the
obs indices by cell id and the running sum of the cell counts, compared exactly.

Analysis: index mode 1 against mode 0 at the bar of test_binned_search_equals_tree_search:
equal solved / accepted-obs / truncation counts and max_p, increments within 1e-9 relative RMS
(the neighbour sets are identical, the order inside a cell differs: tree slots in mode 0, obs
indices in mode 1, which moves only the fp64 sums of the solve), the golden driver cases also
within INCR_TOL of the reference's output.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import DriverCase, increment_rel_rms

pytestmark = pytest.mark.gpu

INCR_TOL = 1e-6
F = np.float32


# ---- bins ----------------------------------------------------------------------------------------
def search_radius():
    """sqrtf(search_r2), search_r2 = gc1999^2, gc1999 = 2 sqrt(10/3) in fp32."""
    gc = F(2.0) * np.sqrt(F(10.0) / F(3.0), dtype=F)
    return np.sqrt(F(gc * gc), dtype=F)


def normalised(xyz, hclr, vclr):
    hinv = F(1.0) / F(F(hclr) * F(1e3))
    with np.errstate(all="ignore"):
        x = (xyz[:, 0] * hinv).astype(F)
        y = (xyz[:, 1] * hinv).astype(F)
        if vclr > 0:
            z = (xyz[:, 2] * (F(1.0) / F(F(vclr) * F(1e3)))).astype(F)
        else:
            z = np.zeros(len(xyz), F)
    return x, y, z


def expected_bins(xyz, hclr, vclr, grid):
    x, y, z = normalised(xyz, hclr, vclr)
    dim3 = vclr > 0

    def cell(v, b0, nb):
        with np.errstate(all="ignore"):
            f = ((v - F(b0)).astype(F) * F(grid.binv)).astype(F)
            c = np.minimum(np.maximum(np.floor(f), F(0.0)), F(nb - 1))
        c[~np.isfinite(f)] = 0
        return c.astype(np.int64)

    fin = np.isfinite(x) & np.isfinite(y) & (np.isfinite(z) if dim3 else True)
    cz = cell(z, grid.z0, grid.nbz) if dim3 else 0
    cid = np.where(fin, cell(x, grid.x0, grid.nbx) + grid.nbx * (cell(y, grid.y0, grid.nby) + grid.nby * cz), 0)
    ncell = grid.nbx * grid.nby * grid.nbz
    order = np.argsort(cid, kind="stable").astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(cid, minlength=ncell))]).astype(np.int32)
    return cid, start, order


def bin_points(kind, n, seed):
    """(n,3) fp32 metres: 200 km x 200 km x 15 km, hclr 12 / vclr 3 km in the callers."""
    rng = np.random.default_rng(seed)
    xyz = np.empty((n, 3), F)
    xyz[:, 0] = rng.uniform(0, 200e3, n)
    xyz[:, 1] = rng.uniform(0, 200e3, n)
    xyz[:, 2] = rng.uniform(0, 15e3, n)
    if kind == "identical":
        xyz[:] = np.array([31e3, 77e3, 4e3], F)
    elif kind == "nonfinite":
        bad = rng.random(n) < 0.05
        vals = np.array([np.nan, np.inf, -np.inf], F)
        xyz[bad, rng.integers(0, 3, bad.sum())] = vals[rng.integers(0, 3, bad.sum())]
    elif kind == "offset":
        xyz += np.array([5e6, -4e6, 0.0], F)
    return xyz


@pytest.fixture(scope="module")
def bcore():
    c = abi.Core(8, device=0)
    yield c
    c.finalize()


NS = [0, 1, 7, 64, 65, 1000, 20000]
DIVS = [1, 2, 4, 8, 0]


def check_bins(c, xyz, hclr, vclr, div):
    grid, start, order = c.bin_index(xyz, hclr, vclr, div)
    ncell = grid.nbx * grid.nby * grid.nbz
    assert 1 <= ncell <= 1 << 22 and (vclr > 0 or grid.nbz == 1)
    assert grid.div == div if div else grid.div in (2, 4)
    cid, estart, eorder = expected_bins(xyz, hclr, vclr, grid)
    np.testing.assert_array_equal(start, estart)
    np.testing.assert_array_equal(order, eorder)
    return grid, cid, start, order


@pytest.mark.parametrize("dim3", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "identical", "nonfinite", "offset"])
def test_bin_index_matches_numpy(bcore, kind, dim3):
    hclr, vclr = 12.0, (3.0 if dim3 else -1.0)
    r = search_radius()
    for n in NS:
        xyz = bin_points(kind, n, seed=100 + n)
        for div in DIVS:
            grid, cid, start, order = check_bins(bcore, xyz, hclr, vclr, div)
            x, y, z = normalised(xyz, hclr, vclr)
            if kind == "nonfinite" and n:
                bad = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
                if n >= 1000:
                    assert bad.any()
                assert (cid[bad] == 0).all()
                assert set(np.flatnonzero(bad)) <= set(order[start[0]:start[1]])
            if kind == "uniform" and n:
                # origin: the finite minima, bitwise; z0 = 0 in 2-D
                want = [x.min(), y.min(), z.min() if dim3 else F(0.0)]
                got = np.array([grid.x0, grid.y0, grid.z0], F)
                np.testing.assert_array_equal(got.view(np.uint32), np.array(want, F).view(np.uint32))
                h = F(r / F(grid.div))
                ext = [float(x.max()) - float(x.min()), float(y.max()) - float(y.min()),
                       float(z.max()) - float(z.min()) if dim3 else 0.0]
                nb = [1 + int(np.floor(e / float(h))) for e in ext]
                if nb[0] * nb[1] * nb[2] <= 1 << 22:  # the cap does not bind
                    assert [grid.nbx, grid.nby, grid.nbz] == nb
                    assert F(grid.binv).view(np.uint32) == F(F(1.0) / h).view(np.uint32)
                if div == 0:  # the density rule: more than 24 obs per r/2 cell -> r/4
                    cells = np.prod([max(1.0, e / (0.5 * float(r))) for e in ext[:3 if dim3 else 2]])
                    assert grid.div == (4 if n / cells > 24.0 else 2)


def test_bin_index_fine_grid_three_sort_passes(bcore):
    """More than 2^16 cells (three 8-bit sort passes) with many points per block."""
    xyz = bin_points("uniform", 20000, seed=7)
    grid, cid, start, order = check_bins(bcore, xyz, 3.0, 1.0, 8)
    assert grid.nbx * grid.nby * grid.nbz > 1 << 16
    grid2, start2, order2 = bcore.bin_index(xyz, 3.0, 1.0, 8)  # a second call: identical arrays
    np.testing.assert_array_equal(start2, start)
    np.testing.assert_array_equal(order2, order)
    assert bytes(grid2) == bytes(grid)


@pytest.mark.parametrize("dim3", [False, True])
def test_bin_index_cell_cap(bcore, dim3):
    """100 points over 3000 r in x and y at div 2: 6000 x 6000 cells of r/2 pass the 2^22 cap,
    so the cells grow (x 1.25 a step) until the grid fits."""
    rng = np.random.default_rng(3)
    hclr, vclr = 12.0, (3.0 if dim3 else -1.0)
    span = 3000.0 * float(search_radius()) * hclr * 1e3
    xyz = np.empty((100, 3), F)
    xyz[:, 0] = rng.uniform(0, span, 100)
    xyz[:, 1] = rng.uniform(0, span, 100)
    xyz[:, 2] = rng.uniform(0, 15e3, 100)
    xyz[0, :2] = 0.0
    xyz[1, :2] = span
    grid, cid, start, order = check_bins(bcore, xyz, hclr, vclr, 2)
    assert grid.nbx * grid.nby * grid.nbz <= 1 << 22
    assert F(grid.binv) < F(1.0) / F(search_radius() / F(2.0))  # grown cells
    assert grid.nbx > 1000 and grid.nby > 1000


def test_bin_index_device_memory_and_grid_only(bcore):
    torch = pytest.importorskip("torch")
    xyz = bin_points("uniform", 1000, seed=9)
    grid, start, order = bcore.bin_index(xyz, 12.0, 3.0, 2)
    g2, s2, o2 = bcore.bin_index(torch.from_numpy(xyz).to("cuda:0"), 12.0, 3.0, 2,
                                 memory=abi.MEM_DEVICE)
    assert bytes(g2) == bytes(grid)
    np.testing.assert_array_equal(s2.cpu().numpy(), start)
    np.testing.assert_array_equal(o2.cpu().numpy(), order)
    g3, s3, o3 = bcore.bin_index(xyz, 12.0, 3.0, 2, grid_only=True)
    assert bytes(g3) == bytes(grid) and s3 is None and o3 is None
    with pytest.raises(abi.CwblError, match="ARG"):  # start too short
        bcore._check(bcore.lib.cwbl_bin_index(1000, xyz.ctypes.data, 12.0, 3.0, 2, C.byref(grid),
                                              3, start.ctypes.data, order.ctypes.data, abi.MEM_HOST))
    with pytest.raises(abi.CwblError, match="ARG"):
        bcore.bin_index(xyz, 12.0, 3.0, 9)


# ---- analysis --------------------------------------------------------------------------------------
class Case:
    """One analysis workload: a golden driver fixture or a synthetic radar set."""

    def __init__(self, name):
        self.name = name
        if name.endswith(".npz"):
            d = DriverCase(name)
            self.k, self.wf, self.norain, self.vp = d.k, d.wf, d.norain, d.vp
            self.obs, self.slab, self.var_in, self.var_out = d.obs_set, d.slab, d.var_in, d.var_out
            self.driver = d
            return
        if name == "c2_truncfree":  # 2025 obs against max_lz 1000, no list near max_lz
            w = synth.make("c2", seed=41, scale=0.3, nz=10)
        else:
            w = synth.make(name[:2], scale=0.04 if name == "c5" else 0.12)
        if name == "c2_far":  # 5000 km off the projection origin, 1.5 km localisation
            w.x = w.x + F(5e6)
            w.y = w.y - F(4e6)
            w.obs_xyz = w.obs_xyz + np.array([5e6, -4e6, 0.0], F)
            for tp in w.vp.radar:
                tp.hclr = tp.hclr / 8.0
        self.w = w
        self.k, self.wf, self.norain, self.vp = w.k, 0, -5.0, w.vp
        self.var_in, self.var_out = w.var, None
        self.obs = lambda: abi.ObsSetBuilder().add_radar(w.radar_type, w.obs_xyz, w.obs,
                                                         w.hdxb).build()

        def slab():
            var = w.var.copy()
            return abi.make_slab(w.x, w.y, w.alt, var), var
        self.slab = slab


_cases, _runs = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def counts(st):
    return (st.solved, st.nobs_sum, st.lz_truncated, st.max_p)


def fresh_core(case, options):
    return abi.Core(case.k, device=0, weight_function=case.wf, norain_value=case.norain,
                    options=options)


def analyse(name, **options):
    """One analysis from a fresh library state: (var, counts, prep info); kept per (case,
    options), read-only for the tests that share it."""
    key = (name, tuple(sorted(options.items())))
    if key not in _runs:
        case = case_of(name)
        c = fresh_core(case, options)
        try:
            c.set_obs(case.obs())
            slab, var = case.slab()
            st = c.analyze_var(case.vp, slab)
            info = c.prep_info().as_dict()
        finally:
            c.finalize()
        var.setflags(write=False)
        _runs[key] = (var, counts(st), info)
    return _runs[key]


CASES = ["driver_mixed.npz", "driver_c1.npz", "driver_q1.npz", "c2", "c2_far", "c5"]


@pytest.mark.parametrize("name", CASES)
def test_device_index_equals_host_index(name):
    case = case_of(name)
    v0, c0, i0 = analyse(name, index=0)
    v1, c1, i1 = analyse(name, index=1)
    assert c1 == c0, (c1, c0)
    assert c0[0] > 0
    rel = increment_rel_rms(v1, v0, case.var_in)
    print(f"{name}: mode 1 vs mode 0 rel rms {rel:.3e}; counts {c1}; prep {i1}")
    assert rel <= 1e-9, rel
    if case.var_out is not None:
        assert increment_rel_rms(v1, case.var_out, case.var_in) <= INCR_TOL
    assert i0["bins_on_device"] == 0 and i0["bins_built"] == i0["trees_built"] > 0
    assert i1["bins_on_device"] == i1["bins_built"] == i0["bins_built"]
    if name == "driver_mixed.npz":  # truncated lists: the tree search ran in mode 1
        assert c1[2] > 0 and i1["flagged_batches"] > 0 and i1["trees_built"] > 0


def test_device_index_with_several_batches():
    case = case_of("driver_mixed.npz")
    v0, c0, _ = analyse("driver_mixed.npz", index=0)
    v1, c1, i1 = analyse("driver_mixed.npz", index=1, max_batch=256)
    assert case.var_in[0].size > 2 * 256  # several batches
    assert c1 == c0
    assert increment_rel_rms(v1, v0, case.var_in) <= 1e-9
    assert increment_rel_rms(v1, case.var_out, case.var_in) <= INCR_TOL
    assert i1["flagged_batches"] > 0


@pytest.mark.parametrize("name", ["driver_mixed.npz", "driver_c1.npz"])
def test_tree_walk_is_bit_identical_in_both_index_modes(name):
    """CWBL_OPT_SEARCH = 1: the lists are in kdtree2's order either way, only the column
    numbering (tree slot / obs index) differs."""
    v0, c0, _ = analyse(name, index=0, search=1)
    v1, c1, i1 = analyse(name, index=1, search=1)
    assert c1 == c0
    np.testing.assert_array_equal(v1.view(np.uint32), v0.view(np.uint32))
    assert i1["trees_built"] > 0 and i1["bins_on_device"] > 0


def test_device_index_repeats_bitwise_from_a_fresh_state():
    name = "driver_mixed.npz"
    v1, c1, _ = analyse(name, index=1)
    case = case_of(name)
    c = fresh_core(case, {"index": 1})
    try:
        c.set_obs(case.obs())
        slab, var = case.slab()
        st = c.analyze_var(case.vp, slab)
    finally:
        c.finalize()
    assert counts(st) == c1
    np.testing.assert_array_equal(var.view(np.uint32), v1.view(np.uint32))


def test_no_tree_when_no_list_can_truncate():
    """324 obs against max_lz 1000: no list can pass max_lz, so no tree is ever built."""
    case = case_of("c2")
    assert case.w.obs.shape[0] == 324 and case.vp.radar[case.w.radar_type - 1].max_lz_pts == 1000
    _, c1, i1 = analyse("c2", index=1)
    assert i1["trees_built"] == 0 and i1["flagged_batches"] == 0 and i1["ms_tree_wait"] == 0
    assert c1[2] == 0


def longest_list(w):
    """Longest fixed-radius list over the grid, fp32 as get_lz computes it."""
    cfg = w.extra["cfg"]
    ox, oy, oz = normalised(w.obs_xyz, cfg["hclr"], cfg["vclr"])
    hinv = F(1.0) / F(F(cfg["hclr"]) * F(1e3))
    vinv = F(1.0) / F(F(cfg["vclr"]) * F(1e3))
    r = search_radius()
    gc = F(2.0) * np.sqrt(F(10.0) / F(3.0), dtype=F)
    r2 = F(gc * gc)
    best = 0
    qx = (w.x * hinv).astype(F)
    qy = (w.y * hinv).astype(F)
    for j in range(w.ny):  # one grid row at a time, every level: only the obs near the row
        near = np.abs(oy - qy[j, 0]) <= r + F(0.01)
        x, y, z = ox[near], oy[near], oz[near]
        qz = (w.alt[:, j, :] * vinv).astype(F).reshape(-1, 1)
        qxx = np.broadcast_to(qx[j], (w.nz, w.nx)).reshape(-1, 1)
        dx, dy, dz = x[None] - qxx, y[None] - qy[j, 0], z[None] - qz
        d2 = ((dx * dx + dy * dy).astype(F) + dz * dz).astype(F)
        best = max(best, int((d2 <= r2).sum(axis=1).max()))
    return best


def test_no_tree_wait_when_no_list_truncates():
    """2025 obs against max_lz 1000 can truncate a priori, so a worker builds the tree; the
    longest list (counted here on the CPU from the fp32-normalised coordinates: 366, and the
    same from an fp64 k-d tree) is far below max_lz, so no batch flags a point and the call
    never waits for the tree."""
    case = case_of("c2_truncfree")
    w = case.w
    max_lz = case.vp.radar[w.radar_type - 1].max_lz_pts
    assert w.obs.shape[0] == 2025 and max_lz == 1000
    longest = longest_list(w)
    assert 0 < longest < max_lz // 2, longest
    _, c0, _ = analyse("c2_truncfree", index=0)
    _, c1, i1 = analyse("c2_truncfree", index=1)
    assert i1["trees_built"] == 0 or i1["ms_tree_wait"] == 0
    assert i1["flagged_batches"] == 0 and c1[2] == 0
    assert c1 == c0 and c1[3] <= longest


def test_device_index_cache():
    """One obs set, mode 1: a repeated call builds no bins and returns the same bits, also with
    a call of another normalisation in between; bin_div 0 -> 1 -> 4 -> 0 rebuilds the bins
    alone, keeps the counts and ends on the first call's bits."""
    name = "driver_mixed.npz"
    case = case_of(name)
    v1, c1, _ = analyse(name, index=1)
    c = fresh_core(case, {"index": 1})
    try:
        c.set_obs(case.obs())

        def call(vp=case.vp):
            slab, var = case.slab()
            st = c.analyze_var(vp, slab)
            return var, counts(st), c.prep_info().as_dict()
        va, ca, ia = call()
        assert ia["bins_built"] > 0 and ia["bins_on_device"] == ia["bins_built"]
        vb, cb, ib = call()
        assert ib["bins_built"] == 0 and ib["trees_built"] == 0 and cb == ca == c1
        np.testing.assert_array_equal(vb.view(np.uint32), va.view(np.uint32))
        np.testing.assert_array_equal(va.view(np.uint32), v1.view(np.uint32))
        other = copy.deepcopy(case.vp)
        for tp in list(other.gts) + list(other.radar):
            tp.hclr = tp.hclr * 1.5
            tp.err_muti[0] = tp.err_muti[0] * 2.0
        _, _, io = call(other)
        assert io["bins_built"] > 0
        vc, cc, ic = call()
        assert ic["bins_built"] == 0 and cc == ca
        np.testing.assert_array_equal(vc.view(np.uint32), va.view(np.uint32))
        outs = []
        for div in (0, 1, 4, 0):
            c.set_option("bin_div", div)
            var, cnt, info = call()
            assert info["trees_built"] == 0  # the trees stay, only the bins follow the divisor
            outs.append((var, cnt, info))
        assert outs[1][2]["bins_built"] > 0 and outs[2][2]["bins_built"] > 0
        for var, cnt, _ in outs:
            assert cnt == ca
            assert increment_rel_rms(var, va, case.var_in) <= 1e-9
        np.testing.assert_array_equal(outs[3][0].view(np.uint32), va.view(np.uint32))
    finally:
        c.finalize()


def test_device_index_device_memory_equals_host_memory():
    torch = pytest.importorskip("torch")
    name = "driver_mixed.npz"
    case = case_of(name)
    d = case.driver
    v1, c1, _ = analyse(name, index=1)
    dev = torch.device("cuda:0")
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    c = fresh_core(case, {"index": 1})
    try:
        c.set_obs(d.obs_set(memory=abi.MEM_DEVICE, to_device=to_dev))
        x, y, alt = (to_dev(np.asarray(a, F)) for a in (d.x, d.y, d.alt))
        var = to_dev(np.asarray(d.var_in, F).copy())
        torch.cuda.synchronize()
        slab = abi.make_slab(x, y, alt, var, d.ix_lim, d.iy_lim, memory=abi.MEM_DEVICE)
        st = c.analyze_var(case.vp, slab)
        got = var.cpu().numpy()
    finally:
        c.finalize()
    assert counts(st) == c1
    np.testing.assert_array_equal(got.view(np.uint32), v1.view(np.uint32))


def test_index_option_range_and_default():
    case = case_of("driver_c1.npz")
    c = fresh_core(case, {"index": 1})
    try:
        with pytest.raises(abi.CwblError, match="ARG"):
            c.set_option("index", 2)
        with pytest.raises(abi.CwblError, match="ARG"):
            c.set_option("index", -1)
    finally:
        c.finalize()
    c = fresh_core(case, None)  # cwbl_init resets the option: a new Core is in mode 0
    try:
        c.set_obs(case.obs())
        slab, var = case.slab()
        c.analyze_var(case.vp, slab)
        info = c.prep_info().as_dict()
    finally:
        c.finalize()
    assert info["bins_built"] > 0 and info["bins_on_device"] == 0
    v0, _, _ = analyse("driver_c1.npz", index=0)
    np.testing.assert_array_equal(var.view(np.uint32), v0.view(np.uint32))
