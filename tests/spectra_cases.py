"""The wide-spectrum workloads of tests/test_gpu_analyze_vars_spectra.py and what the CPU knows
about them: every point's quadrature level (helpers.quad_level of the fp64 spectrum bound), the
fp64 truth (helpers.eigen_direct_solve) and that truth's own floor (the same evaluation with the
columns in reversed order).  tests/test_truth_spectra.py asserts the input conditions here,
without a GPU; the GPU tests assert them again on the level map they compare the counters with.

Workload: pair_ensemble(synth c2, 12 x 12 x 5 = 720 points, n_obs obs, k members) at obs error
2^e.  With 120 obs every point sees p = 36..120 obs, with 12 obs p = 3..12 (p < k at every k);
k = 96 and 128 take 250 obs for their dense cases (Case.tol below).  The level of a point is
set by the obs error and p and hardly by k (the columns' norms and inflat both grow with k),
so one table of errors serves every k:

  n_obs     err     levels          R of the record path      passes elsewhere
  120       2^-3    3, 4, 5         2 and 3                   (record path only)
  120, 250  2^-10   7, 8, 9         4                         1
  120, 250  2^-16   11, 12, 13      4 and 8, mixed in fours   1 and 2, among neighbours
  120, 250  2^-19   13, 14 (, 15)   8                         2
  12        2^-6    4, 5, 6         3 and 4, mixed in fours   (record path only)
  12        2^-18   11, 12, 13      4 and 8, mixed in fours   1 and 2, among neighbours
"""
import functools
from collections import namedtuple

import numpy as np

from cwbl import synth
from helpers import (eigen_direct_solve, inflat_of, near_decade, pair_ensemble, quad_level,
                     quad_passes, quad_rounds, radar_point_columns, spectrum_ratio)

INCR_TOL = 1e-6

#: classes: the R (record path, k = 32) or pass counts (every other k) the case must contain;
#: mixed: two classes inside one aligned group of four consecutive points (a wave of
#: solve_tq40_multi_kernel), which are neighbouring points for the other kernels;
#: tol: the truth bound in units of INCR_TOL.  It is 1 where the fp64 floor of the truth (the
#: reversed-column evaluation) is <= INCR_TOL / 4, which the dense cases reach: at k = 96 and
#: 128 with 250 obs instead of 120 (with 120 the floor is 4.5e-7 at 2^-16 and 1.2e-5..2.2e-5
#: at 2^-19, with 250 the two evaluations agree in every fp32 bit).  The sparse cases at 2^-18
#: cannot reach it at any size: p < k is what they are for, and the unobserved antisymmetric
#: directions (eigenvalue inflat next to |A| ~ 1e13 inflat) are resolved to eps |A| / inflat
#: by everything that forms A in fp64.  There the bound is the smallest multiple of INCR_TOL
#: >= 4 x the floor measured on the CPU (SPARSE_FLOORS, asserted by test_truth_spectra).
Case = namedtuple("Case", "k n_obs e classes mixed tol")

#: measured floor / deviation of the oracle from the truth, sparse cases at 2^-18
SPARSE_FLOORS = {16: (1.13e-6, 6.88e-6), 32: (2.55e-5, 2.96e-5), 64: (3.58e-5, 5.10e-5),
                 96: (7.23e-5, 7.98e-5), 128: (9.39e-5, 1.12e-4)}
SPARSE_TOL = {16: 5, 32: 103, 64: 144, 96: 290, 128: 376}

RECORD = [Case(32, 120, -3, (2, 3), False, 1), Case(32, 120, -10, (4,), False, 1),
          Case(32, 120, -16, (4, 8), True, 1), Case(32, 120, -19, (8,), False, 1),
          Case(32, 12, -6, (3, 4), True, 1), Case(32, 12, -18, (4, 8), True, SPARSE_TOL[32])]
WAVE = [Case(k, n, e, c, m, SPARSE_TOL[k] if n == 12 else 1) for k in (16, 64)
        for n, e, c, m in ((120, -10, (1,), False), (120, -16, (1, 2), True),
                           (120, -19, (2,), False), (12, -18, (1, 2), True))]
BIG = [Case(k, n, e, c, m, SPARSE_TOL[k] if n == 12 else 1) for k in (128, 96)
       for n, e, c, m in ((250, -10, (1,), False), (250, -16, (1, 2), True),
                          (250, -19, (2,), False), (12, -18, (1, 2), True))]
CASES = RECORD + WAVE + BIG


def case_id(c):
    return f"k{c.k}-n{c.n_obs}-e{-c.e}"


def on_record_path(k):
    return 17 <= k <= 40


def workload(c):
    return pair_ensemble(synth.make("c2", nx=12, ny=12, nz=5, n_obs=c.n_obs, k=c.k), 2.0 ** c.e)


def class_of(k, level):
    return quad_rounds(level) if on_record_path(k) else quad_passes(level)


def means_exact(w):
    """True when fl(sum over the members, in order) * fl(1/k) gives back the dyadic member mean
    exactly, for every obs column of hdxb and every point of var: the perturbations are then
    exactly zero-sum.  A power of two k has it by construction; k = 96 has it because fl(1/96)
    is off by +2^-26.6 relative, less than half an ulp of the means used.  Checked, not assumed."""
    ok = True
    for a in (w.hdxb, w.var.reshape(w.k, -1)):
        s = np.zeros(a.shape[1], np.float32)
        for m in range(w.k):
            s = (s + a[m]).astype(np.float32)
        mean = (s * np.float32(1.0 / w.k)).astype(np.float32)
        pair = ((a[0::2].astype(np.float64) + a[1::2]) / 2.0)  # every pair's midpoint
        ok = ok and bool(np.all(pair == mean.astype(np.float64)[None]))
    return ok


Evaluation = namedtuple("Evaluation", "levels near truth truth_rev")


@functools.lru_cache(maxsize=4)
def evaluate(c, floor=False):
    """Per point of the case: the level (0 where p = 0), whether the ratio lies within 1e-9 of
    a decade, the fp64 truth of variable 0 and, floor=True, the truth from the reversed
    columns (else None).  Arrays of the slab's shape, point index g = i + nx (j + ny kz)."""
    w = workload(c)
    vp = w.vp
    infl = inflat_of(c.k, vp.multi_infl)
    nz, ny, nx = w.var.shape[1:]
    levels = np.zeros((nz, ny, nx), np.int32)
    near = np.zeros((nz, ny, nx), bool)
    truth = w.var.copy()
    rev = w.var.copy() if floor else None
    for kz in range(nz):
        for j in range(ny):
            for i in range(nx):
                yo, yb = radar_point_columns(w, kz, j, i, 2.0 ** c.e)
                if not len(yo):
                    continue
                ratio = spectrum_ratio(yb, infl)
                levels[kz, j, i] = quad_level(ratio)
                near[kz, j, i] = near_decade(ratio)
                args = (infl, vp.use_rtpp, vp.rtpp_alpha, vp.use_rtps, vp.rtps_alpha)
                truth[:, kz, j, i] = eigen_direct_solve(c.k, w.var[:, kz, j, i], yo, yb, *args)
                if floor:
                    rev[:, kz, j, i] = eigen_direct_solve(c.k, w.var[:, kz, j, i], yo[::-1],
                                                          yb[::-1], *args)
    return Evaluation(levels, near, truth, rev)


def classes_present(c, levels):
    lv = levels.ravel()
    return sorted({class_of(c.k, int(v)) for v in lv if v > 0})


def mixed_fours(c, levels):
    """Aligned groups of four consecutive point indices that hold two classes."""
    cl = np.array([class_of(c.k, int(v)) if v > 0 else 0 for v in levels.ravel()]).reshape(-1, 4)
    return int(sum(len(set(r.tolist()) - {0}) > 1 for r in cl))


def ulp_floor(truth, var):
    """The fp32 rounding floor of the increments: one ulp of xa at every updated value, as a
    fraction of the rms increment (tests/test_gpu_parity.py, the tiny-obs-error test)."""
    upd = truth != var
    return float(np.sqrt(np.mean(np.spacing(np.abs(truth[upd])).astype(np.float64) ** 2)) /
                 np.sqrt(np.mean((truth[upd].astype(np.float64) - var[upd]) ** 2)))
