"""GPU tests of cwbl_analyze_vars (Core.analyze_vars): the variables of a group, which share
the obs, the localisation, multi_infl and the grid, analysed in one call.

On the k = 17..40 record path the call searches and assembles once per batch and runs
solve_tq40_multi_kernel, which tridiagonalises once per point and replays the reflectors on
every variable's x'.  The replay evaluates the expressions of solve_tq40_kernel, so every
comparison with the per-variable calls (`seq`: cwbl_analyze_var per variable on a fresh core)
is exact: np.array_equal on the bit patterns, plus the counters.  Here only the oracle
comparison has a tolerance, the project's path-versus-oracle bar INCR_TOL, and every input is
the benign c2 one (levels 1..3, one radar type, Gaussian weights): the wide spectra, the fp64
truth, non-finite variables and the reference's mixed-obs cases are in
tests/test_gpu_analyze_vars_spectra.py and tests/test_gpu_analyze_vars_golden.py.

Workload: synth c2 at scale 0.1 (30 x 30 x 50 = 45 000 points, k = 40, 225 obs) in search
batches of 1024 points and record sub-batches of 512: 44 batches of two sub-batches, without
the record cache (record_reuse = 0) unless a test says otherwise.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from cwbl import abi, synth
from helpers import increment_rel_rms, oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INCR_TOL = 1e-6
OPTS = {"max_batch": 1024, "split40_batch": 512, "record_reuse": 0}
COUNTERS = ("points", "solved", "nobs_sum", "lz_truncated", "nonconverged", "q1_undefined",
            "sweeps_sum", "max_p", "max_sweeps", "ntrees")
MULTI = "solve_tq40_multi_kernel<40>"
ASSEMBLE = "assemble_record_kernel<4>"


def counters(st):
    return {n: getattr(st, n) for n in COUNTERS}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def other_var(w, seed):
    """Another variable on the same grid: the same shape, other values."""
    rng = np.random.default_rng(seed)
    return (w.var + rng.standard_normal(w.var.shape, dtype=np.float32)).astype(np.float32)


def variables(w, n):
    return [w.var] + [other_var(w, 100 + i) for i in range(1, n)]


class Lib:
    """One library state with the workload's obs set and its coordinates on the device (or,
    host=True, in pageable numpy arrays): one set of x, y, alt arrays for every slab."""

    def __init__(self, w, opts=None, host=False, reuse_default=False, weight_function=0,
                 norain_value=-5.0, obs_set=None):
        """obs_set: a built cwbl_obs_set instead of the workload's one radar type."""
        options = dict(OPTS)
        if reuse_default:
            del options["record_reuse"]
        options.update(opts or {})
        self.w, self.host = w, host
        self.c = abi.Core(w.k, device=0, weight_function=weight_function,
                          norain_value=norain_value, options=options)
        self.c.set_obs(obs_set if obs_set is not None else abi.ObsSetBuilder().add_radar(
            w.radar_type, w.obs_xyz, w.obs, w.hdxb).build())
        self.x, self.y, self.alt = (a.copy() if host else to_dev(a) for a in (w.x, w.y, w.alt))

    def slab(self, v, ix_lim=None, alt=None, iy_lim=None):
        return abi.make_slab(self.x, self.y, self.alt if alt is None else alt, v, ix_lim=ix_lim,
                             iy_lim=iy_lim, memory=abi.MEM_HOST if self.host else abi.MEM_DEVICE)

    def buffers(self, vars_):
        if self.host:
            return [np.array(v, np.float32, copy=True) for v in vars_]
        bufs = [to_dev(v) for v in vars_]
        torch.cuda.synchronize()
        return bufs

    @staticmethod
    def fetch(b):
        return b if isinstance(b, np.ndarray) else b.cpu().numpy()

    def one(self, var, vp, ix_lim=None, iy_lim=None):
        """cwbl_analyze_var on a copy of var: (analysis, counters)."""
        b, = self.buffers([var])
        st = self.c.analyze_var(vp, self.slab(b, ix_lim, iy_lim=iy_lim))
        return self.fetch(b), counters(st)

    def group(self, vars_, vps, ix_lim=None, iy_lim=None):
        """cwbl_analyze_vars on copies of vars_: ([analysis], counters)."""
        bufs = self.buffers(vars_)
        st = self.c.analyze_vars(vps, [self.slab(b, ix_lim, iy_lim=iy_lim) for b in bufs])
        return [self.fetch(b) for b in bufs], counters(st)

    def close(self):
        self.c.finalize()


def seq(w, vars_, vps, opts=None, ix_lim=None, **core):
    """cwbl_analyze_var per variable on a fresh core: [(analysis, counters)]."""
    lib = Lib(w, opts, **core)
    try:
        return [lib.one(v, vp, ix_lim) for v, vp in zip(vars_, vps)]
    finally:
        lib.close()


def group(w, vars_, vps, opts=None, ix_lim=None, host=False, **core):
    lib = Lib(w, opts, host=host, **core)
    try:
        return lib.group(vars_, vps, ix_lim)
    finally:
        lib.close()


def same_as_seq(got, want):
    """A group call's ([analysis], counters) against seq's [(analysis, counters)]."""
    outs, cnt = got
    assert len(outs) == len(want)
    for i, (out, (ref, rcnt)) in enumerate(zip(outs, want)):
        assert cnt == rcnt, (i, cnt, rcnt)
        assert np.array_equal(bits(out), bits(ref)), i


@functools.lru_cache(maxsize=None)
def workload():
    return synth.make("c2", scale=0.1)


@functools.lru_cache(maxsize=None)
def seq8():
    """The per-variable analyses of the eight variables of the main workload, computed once."""
    w = workload()
    return seq(w, variables(w, 8), [w.vp] * 8)


@pytest.mark.parametrize("nvar", [1, 2, 3, 8])
def test_group_equals_sequential(nvar):
    w = workload()
    vars_ = variables(w, nvar)
    ref = seq8()[:nvar]
    assert ref[0][1]["solved"] > 0
    lib = Lib(w)
    try:
        lib.c.set_kernel_timing(True)
        got = lib.group(vars_, [w.vp] * nvar)
        kt = lib.c.kernel_times()
        info = lib.c.reuse_info().as_dict()
    finally:
        lib.close()
    same_as_seq(got, ref)
    for i in range(nvar):
        for j in range(i + 1, nvar):
            assert not np.array_equal(bits(got[0][i]), bits(got[0][j])), (i, j)
    assert kt[MULTI]["points"] == w.points, kt
    assert kt[MULTI]["launches"] == 88, kt  # 44 batches of two sub-batches, whatever nvar
    assert kt[ASSEMBLE]["points"] == w.points, kt
    assert not [n for n in kt if n.startswith("solve_tq40_kernel")], kt
    assert info["batches_reused"] == 0 and info["batches_assembled"] == 44, info
    assert info["bytes_held"] == 0, info


def test_per_variable_epilogue():
    """RTPP only, RTPS only, both with tune_q, neither: each variable's own flags and alphas."""
    w = workload()
    vps = [copy.deepcopy(w.vp) for _ in range(4)]
    vps[0].use_rtpp, vps[0].rtpp_alpha, vps[0].use_rtps = 1, 0.5, 0
    vps[1].use_rtpp, vps[1].use_rtps, vps[1].rtps_alpha = 0, 1, 0.7
    vps[2].use_rtpp, vps[2].rtpp_alpha, vps[2].use_rtps, vps[2].rtps_alpha = 1, 0.5, 1, 0.7
    vps[2].tune_q = 1
    vps[3].use_rtpp, vps[3].use_rtps = 0, 0
    vars_ = variables(w, 4)
    ref = seq(w, vars_, vps)
    # the settings matter: the same variable under another variable's settings differs
    other = seq(w, [vars_[0]], [vps[3]])
    assert not np.array_equal(bits(ref[0][0]), bits(other[0][0]))
    same_as_seq(group(w, vars_, vps), ref)


def test_group_vs_oracle():
    w = workload()
    vars_ = variables(w, 3)
    outs, cnt = group(w, vars_, [w.vp] * 3)
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
        differ = np.count_nonzero(bits(out) != bits(ref))
        print(f"increment_rel_rms vs oracle: {rel:.3e} ({differ} of {moved} analysed values "
              f"differ in their bits, rms increment {np.sqrt(np.mean((ref - var) ** 2)):.3e})")
        assert moved > 0
        assert rel <= INCR_TOL, rel


@functools.lru_cache(maxsize=None)
def _ragged_cases():
    from test_gpu_record_reuse import _ragged_cases as cases
    return dict(cases())


@pytest.mark.parametrize("case", ["k25", "k33", "spare", "sparse"])
def test_ragged_and_sparse(case):
    """Padding rows (k = 25, 33), the spare record (points % 4 == 1) and points with p = 0 and
    p < k (every 25th obs)."""
    wl = _ragged_cases()[case]
    if case == "spare":
        assert wl.points % 4 == 1
    vars_ = variables(wl, 3)
    ref = seq(wl, vars_, [wl.vp] * 3)
    got = group(wl, vars_, [wl.vp] * 3)
    same_as_seq(got, ref)
    if case == "sparse":
        assert 0 < ref[0][1]["solved"] < wl.points          # points with p = 0
        assert ref[0][1]["nobs_sum"] / ref[0][1]["solved"] < wl.k  # and with p < k
        for out, var in zip(got[0], vars_):  # they stay untouched in every variable
            untouched = np.all(bits(out) == bits(var), axis=0)
            assert untouched.sum() == wl.points - ref[0][1]["solved"]


def test_staggered():
    w = workload()
    vars_ = variables(w, 2)
    ref = seq(w, vars_, [w.vp] * 2, ix_lim=w.nx - 1)
    got = group(w, vars_, [w.vp] * 2, ix_lim=w.nx - 1)
    same_as_seq(got, ref)
    assert got[1]["points"] == (w.nx - 1) * w.ny * w.nz
    for out, var in zip(got[0], vars_):  # the last column is not analysed
        assert np.array_equal(bits(out[..., -1]), bits(var[..., -1]))


def test_host_slabs():
    """Pageable numpy slabs: equal to the device-slab result."""
    w = workload()
    same_as_seq(group(w, variables(w, 3), [w.vp] * 3, host=True), seq8()[:3])


@pytest.mark.parametrize("window", [256, 2500])
def test_info_window(window):
    w = workload()
    same_as_seq(group(w, variables(w, 2), [w.vp] * 2, opts={"info_window": window}), seq8()[:2])


def test_cache_untouched():
    """record_reuse at its default: a miss fills the cache, the group call neither reads nor
    touches it, the next cwbl_analyze_var is a full hit."""
    w = workload()
    vars_ = variables(w, 4)
    ref = seq8()
    lib = Lib(w, reuse_default=True)
    try:
        out, cnt = lib.one(vars_[0], w.vp)
        fill = lib.c.reuse_info().as_dict()
        assert fill["batches_reused"] == 0 and fill["batches_assembled"] == 44, fill
        assert fill["bytes_held"] > 0, fill
        assert cnt == ref[0][1] and np.array_equal(bits(out), bits(ref[0][0]))
        same_as_seq(lib.group(vars_[1:4], [w.vp] * 3), ref[1:4])
        info = lib.c.reuse_info().as_dict()
        assert info["batches_reused"] == 0 and info["batches_assembled"] == 44, info
        assert info["bytes_held"] == fill["bytes_held"], (info, fill)
        out, cnt = lib.one(vars_[1], w.vp)
        hit = lib.c.reuse_info().as_dict()
        assert hit["batches_reused"] == 44 and hit["batches_assembled"] == 0, hit
        assert cnt == ref[1][1] and np.array_equal(bits(out), bits(ref[1][0]))
    finally:
        lib.close()


FALLBACKS = {"k8": (8, {}), "k64": (64, {}), "k128": (128, {}),
             "k40_split40_0": (40, {"split40": 0}), "k40_solver_1": (40, {"solver": 1})}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_paths(case):
    """Outside the record path the variables run one after another through cwbl_analyze_var."""
    k, opts = FALLBACKS[case]
    wl = synth.make("c2", nx=12, ny=12, nz=5, n_obs=120, k=k)
    vars_ = variables(wl, 2)
    ref = seq(wl, vars_, [wl.vp] * 2, opts=opts)
    assert ref[0][1]["solved"] > 0
    lib = Lib(wl, opts)
    try:
        lib.c.set_kernel_timing(True)
        got = lib.group(vars_, [wl.vp] * 2)
        kt = lib.c.kernel_times()
    finally:
        lib.close()
    same_as_seq(got, ref)
    assert MULTI not in kt, kt


def test_argument_errors():
    w = workload()
    vars_ = variables(w, 2)
    lib = Lib(w)
    try:
        bufs = lib.buffers(vars_ + [vars_[0]] * 7)

        def unmodified():
            torch.cuda.synchronize()
            for b, v in zip(bufs, vars_ + [vars_[0]] * 7):
                assert np.array_equal(bits(b.cpu().numpy()), bits(v))

        def refused(vps, slabs, what):
            with pytest.raises(abi.CwblError, match="ARG") as e:
                lib.c.analyze_vars(vps, slabs)
            assert what in str(e.value), e.value
            unmodified()

        refused([], [], "nvar")
        refused([w.vp] * 9, [lib.slab(b) for b in bufs], "nvar")
        vp2 = copy.deepcopy(w.vp)
        vp2.multi_infl = 1.1
        refused([w.vp, vp2], [lib.slab(b) for b in bufs[:2]], "variable 1 differs from variable 0 in multi_infl")
        vp2 = copy.deepcopy(w.vp)
        vp2.radar[w.radar_type - 1].hclr = 10.0
        refused([w.vp, vp2], [lib.slab(b) for b in bufs[:2]], "variable 1 differs from variable 0 in radar")
        refused([w.vp] * 2, [lib.slab(bufs[0]), lib.slab(bufs[1], ix_lim=w.nx - 1)],
                "variable 1 differs from variable 0 in ix_lim")
        alt2 = lib.alt.clone()  # another array of equal values
        refused([w.vp] * 2, [lib.slab(bufs[0]), lib.slab(bufs[1], alt=alt2)],
                "variable 1 differs from variable 0 in alt")
        refused([w.vp] * 2, [lib.slab(bufs[0]), lib.slab(bufs[0])], "variables 0 and 1 overlap")
        # two views of one allocation, the second starting one level into the first
        k, nz, ny, nx = w.var.shape
        flat = torch.zeros(w.var.size + ny * nx, dtype=torch.float32, device="cuda:0")
        va = flat[:w.var.size].view(k, nz, ny, nx)
        vb = flat[ny * nx:].view(k, nz, ny, nx)
        refused([w.vp] * 2, [lib.slab(va), lib.slab(vb)], "variables 0 and 1 overlap")
        assert float(flat.abs().max()) == 0.0
        # the core is usable after the refusals
        same_as_seq(lib.group(vars_, [w.vp] * 2), seq8()[:2])
    finally:
        lib.close()
