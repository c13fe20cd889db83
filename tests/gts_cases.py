"""A synthetic workload of multi-variable GTS obs types next to one radar type (not a test
module): what tests/test_gts_cases.py checks on the oracle alone and
tests/test_gpu_gts_large_k.py runs through every path of k = 33..128.

Grid and VR obs: synth c2 on 12 x 12 x 5 = 720 points (24 km x 24 km, levels 20 m .. 20 km)
with 150 VR obs.  GTS types in ObsSetBuilder.add_gts's layouts (xyz (nobs, 3), obs / error
(nobs, nvar), hdxb / qc (k, nobs, nvar)), uniform in the domain:

  SOUND  nvar 4, 3-D (vclr 2 km), altitudes over the whole column, 60 obs, is_assim 1 1 0 1
  SYNOP  nvar 5, vclr = -1, 80 obs, is_assim 1 0 1 1 1
  GPSPW  nvar 1, vclr = -1, 40 obs
  METAR  nvar 5, 3-D, 70 obs (q1_undef only)
  SHIPS  three variables, vclr = -1, 50 obs (nvar3 only)

Per (obs, variable) column: 15 % have every member's qc = -1 (dropped), 20 % have some members'
qc = -1 and at least one >= 0 (kept), 5 % are gross errors (obs += 100, rejected by err_rej);
errors are uniform in 0.5 .. 2; err_muti and err_rej differ per variable, and one err_rej of
SOUND and of SYNOP is small enough to reject ordinary departures too.  hclr is 1.8 .. 2.5 km (a
ball of 6.6 .. 9.1 km) and vclr 1.5 .. 2 km, so the neighbour lists differ from point to point.
The positions and the QC / gross-error draws do not depend on k; the values do.

Variants (VARIANTS), each a parameter of make():

  base          SOUND, SYNOP, GPSPW, VR under Q1_REPLICATE: the GTS family is 2-D (GPSPW is its
                last type), so SOUND is searched in 2-D and queried with its own vclr; 4 trees
  per_type      the same under Q1_PER_TYPE: SOUND searched in 3-D
  q1_undef      SYNOP (2-D), METAR (3-D, the family's last type), VR: SYNOP is the Q1 undefined
                case at every point; 3 trees
  truncated     base with max_lz_pts = 6 for every type
  gaspari_cohn  base with weight_function = 1: NaN points (Q8)
  dense         base with ten times the GTS obs: several chunks per tree on every stager
  sparse        SOUND (6 obs) and every 10th VR obs, both 3-D: points with no neighbour and
                points with p < k; 2 trees
  flat          SYNOP and GPSPW only: every used type is 2-D (column-share eligible); 2 trees
  nvar3         base plus SHIPS with three variables; 5 trees

What the oracle counts at k = 96 (tests/test_gts_cases.py asserts the conditions, not these
numbers): base solves all 720 points with mean p 112 and max p 176 (nobs_sum 80 329; 102 069
without the QC and gross-error rejects), per_type nobs_sum 62 267, q1_undef q1_undefined 720,
truncated lz_truncated 2589, gaspari_cohn 415 NaN points and 305 finite ones, dense mean p 1032
and max p 1515, sparse 577 points solved with mean p 3.9, flat mean p 55; SYNOP gives up to 115
(obs, variable) pairs per point.
"""
import copy
import ctypes as C
import dataclasses
import functools

import numpy as np

from cwbl import abi, synth
from helpers import oracle

SEED = 20261021
NORAIN = -5.0
VARIANTS = ("base", "per_type", "q1_undef", "truncated", "gaspari_cohn", "dense", "sparse",
            "flat", "nvar3")

#: type id: (nvar, obs of the base case, hclr km, vclr km, err_muti, err_rej, is_assim)
GTS = {
    abi.GTS_SOUND: (4, 60, 2.5, 2.0, (1.0, 1.3, 0.8, 1.6), (5.0, 0.7, 6.0, 4.0), (1, 1, 0, 1)),
    abi.GTS_SYNOP: (5, 80, 1.8, -1.0, (1.2, 0.9, 1.0, 1.5, 0.7), (4.0, 5.0, 0.8, 6.0, 3.0),
                    (1, 0, 1, 1, 1)),
    abi.GTS_GPSPW: (1, 40, 2.5, -1.0, (1.1,), (4.5,), (1,)),
    abi.GTS_METAR: (5, 70, 2.0, 2.0, (0.8, 1.1, 1.4, 1.0, 1.2), (5.0, 3.5, 4.0, 0.9, 6.0),
                    (1, 1, 1, 1, 1)),
    abi.GTS_SHIPS: (3, 50, 2.5, -1.0, (1.0, 1.4, 0.9), (4.0, 0.8, 5.0), (1, 1, 1)),
}
VR = dict(hclr=2.5, vclr=1.5, err_muti=1.0, err_rej=8.0)
TYPES = {"q1_undef": (abi.GTS_SYNOP, abi.GTS_METAR), "sparse": (abi.GTS_SOUND,),
         "flat": (abi.GTS_SYNOP, abi.GTS_GPSPW),
         "nvar3": (abi.GTS_SOUND, abi.GTS_SYNOP, abi.GTS_GPSPW, abi.GTS_SHIPS)}
BASE_TYPES = (abi.GTS_SOUND, abi.GTS_SYNOP, abi.GTS_GPSPW)


@dataclasses.dataclass
class Case:
    """One variant at one k: what Lib (test_gpu_analyze_vars) reads of a workload (k, x, y, alt,
    var), the call's parameters and the obs types' arrays."""
    variant: str
    k: int
    nx: int
    ny: int
    nz: int
    x: np.ndarray
    y: np.ndarray
    alt: np.ndarray
    var: np.ndarray
    vp: object
    gts: dict            # type id: (xyz, obs, error, hdxb, qc)
    radar: tuple         # (xyz, obs, hdxb) of VR, or None
    weight_function: int = 0
    q1_mode: int = abi.Q1_REPLICATE

    @property
    def points(self):
        return self.nx * self.ny * self.nz

    def obs_set(self, memory=abi.MEM_HOST, to_device=None):
        """The cwbl_obs_set; to_device(array) for MEM_DEVICE (qc goes as int32)."""
        dev = to_device or (lambda a: a)
        b = abi.ObsSetBuilder(memory)
        for tid, arrays in self.gts.items():
            b.add_gts(tid, *(dev(a) for a in arrays))
        if self.radar is not None:
            b.add_radar(abi.RADAR_VR, *(dev(a) for a in self.radar))
        return b.build()


def _truth(xyz, v):
    """A smooth field per variable, of order one."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return 2.0 * np.sin(x / 9e3 + v) * np.cos(y / 7e3) + 0.5 * np.cos(z / 3.3e3 + 0.3 * v)


def _gts_type(tid, nobs, k, ext, ztop):
    """The arrays of one GTS type.  Geometry, QC classes and gross errors from a stream that
    does not see k; values from one that does."""
    nvar = GTS[tid][0]
    geo = np.random.default_rng([SEED, tid, nobs])
    val = np.random.default_rng([SEED, tid, nobs, k])
    xyz = np.empty((nobs, 3), np.float32)
    xyz[:, 0] = geo.uniform(0, ext[0], nobs)
    xyz[:, 1] = geo.uniform(0, ext[1], nobs)
    xyz[:, 2] = geo.uniform(0, ztop, nobs)
    kind = geo.uniform(size=(nobs, nvar))      # < .15 dropped, < .35 partly flagged
    gross = geo.uniform(size=(nobs, nvar)) < 0.05
    t = np.stack([_truth(xyz, v) for v in range(nvar)], axis=1)
    obs = t + val.standard_normal((nobs, nvar))
    obs[gross] += 100.0
    error = val.uniform(0.5, 2.0, (nobs, nvar))
    hdxb = t[None] + 2.0 * val.standard_normal((k, nobs, nvar))
    qc = val.integers(0, 3, (k, nobs, nvar))
    qc[:, kind < 0.15] = -1
    part = (kind >= 0.15) & (kind < 0.35)
    flagged = val.uniform(size=(k, nobs, nvar)) < 0.5
    flagged[val.integers(0, k), :, :] = False   # at least one member stays >= 0
    qc[flagged & part[None]] = -1
    return (xyz, obs.astype(np.float32), error.astype(np.float32), hdxb.astype(np.float32),
            qc.astype(np.int32))


@functools.lru_cache(maxsize=None)
def make(variant, k):
    """The case of a variant at ensemble size k; shared, never modified."""
    assert variant in VARIANTS, variant
    w = synth.make("c2", nx=12, ny=12, nz=5, n_obs=150, k=k)
    ext = (w.nx * 2e3, w.ny * 2e3)
    max_lz = 6 if variant == "truncated" else 1000
    times = 10 if variant == "dense" else 1
    gts, gts_tp = {}, {}
    for tid in TYPES.get(variant, BASE_TYPES):
        nvar, nobs, hclr, vclr, err_muti, err_rej, is_assim = GTS[tid]
        nobs = 6 if variant == "sparse" else nobs * times
        gts[tid] = _gts_type(tid, nobs, k, ext, 20e3)
        gts_tp[tid] = abi.type_params(use_it=1, max_lz_pts=max_lz, hclr=hclr, vclr=vclr,
                                      err_muti=list(err_muti), err_rej=list(err_rej),
                                      is_assim=list(is_assim))
    radar, radar_tp = None, {}
    if variant != "flat":
        step = 10 if variant == "sparse" else 1
        radar = (np.ascontiguousarray(w.obs_xyz[::step]), np.ascontiguousarray(w.obs[::step]),
                 np.ascontiguousarray(w.hdxb[:, ::step]))
        radar_tp[abi.RADAR_VR] = abi.type_params(use_it=1, max_lz_pts=max_lz, **VR)
    vp = abi.var_params(multi_infl=1.6, use_rtpp=1, rtpp_alpha=0.95, use_rtps=1, rtps_alpha=0.95,
                        gts=gts_tp, radar=radar_tp)
    return Case(variant, k, w.nx, w.ny, w.nz, w.x, w.y, w.alt, w.var, vp, gts, radar,
                weight_function=1 if variant == "gaspari_cohn" else 0,
                q1_mode=abi.Q1_PER_TYPE if variant == "per_type" else abi.Q1_REPLICATE)


def oracle_run(case, var, threads=16):
    """orc_analyze_var on a copy of var: (analysis, Stats)."""
    ref = np.array(var, np.float32, copy=True)
    st = abi.Stats()
    ob = case.obs_set()
    rc = oracle().orc_analyze_var(case.k, case.weight_function, NORAIN, case.q1_mode,
                                  C.byref(ob), C.byref(case.vp),
                                  C.byref(abi.make_slab(case.x, case.y, case.alt, ref)), threads,
                                  C.byref(st))
    assert rc == 0
    return ref, st


@functools.lru_cache(maxsize=None)
def oracle_ref(variant, k):
    """The oracle's analysis of the case's own var and its counters; shared, never modified."""
    case = make(variant, k)
    return oracle_run(case, case.var)


def no_rejects(case):
    """The case with err_rej = 1e30 and every qc = 0: nothing but is_assim removes a column."""
    c = copy.copy(case)
    c.vp = copy.deepcopy(case.vp)
    for tid in case.gts:
        for v in range(abi.MAX_NVAR):
            c.vp.gts[tid - 1].err_rej[v] = 1e30
    c.gts = {tid: a[:4] + (np.zeros_like(a[4]),) for tid, a in case.gts.items()}
    return c


def all_assimilated(case):
    """The case with is_assim = 1 for every variable of every GTS type."""
    c = copy.copy(case)
    c.vp = copy.deepcopy(case.vp)
    for tid in case.gts:
        for v in range(abi.MAX_NVAR):
            c.vp.gts[tid - 1].is_assim[v] = 1
    return c


def pair_counts(case, tid):
    """(obs, variable) pairs per grid point of GTS type tid as the stagers count them: the
    type's neighbours in its own ball (2-D when its vclr <= 0) times nvar."""
    xyz = case.gts[tid][0]
    tp = case.vp.gts[tid - 1]
    q = np.stack([np.broadcast_to(case.x, case.alt.shape).ravel(),
                  np.broadcast_to(case.y, case.alt.shape).ravel(), case.alt.ravel()],
                 axis=1).astype(np.float32)
    cap = xyz.shape[0]
    nf = np.empty(q.shape[0], np.int32)
    idx = np.empty((q.shape[0], cap), np.int32)
    r2 = np.empty((q.shape[0], cap), np.float32)
    oracle().orc_search(xyz.shape[0], xyz.ctypes.data, tp.hclr, tp.vclr, cap, q.shape[0],
                        q.ctypes.data, nf.ctypes.data, idx.ctypes.data, r2.ctypes.data)
    return nf.astype(np.int64) * GTS[tid][0]
