"""CPU-side pins of tests/test_gpu_analyze_vars_spectra.py: the level restatement of
tests/helpers.py against cwbl_internal.h, and the conditions every parametrised case of the GPU
test rests on (tests/spectra_cases.py), checked without a GPU: the R / pass classes present, the
mixed groups of four where claimed, no spectrum bound within 1e-9 of a decade, exact member
means (k = 96 included) and the fp64 floor of the truth the GPU is held to."""
import os
import re

import numpy as np
import pytest

import spectra_cases as sc
from helpers import (QUAD_LEVELS, QUAD_LEVELS_31, REPO, increment_rel_rms, near_decade,
                     quad_level, quad_passes, quad_rounds)

HEADER = os.path.join(REPO, "cwbnwp-letkf_amd", "csrc", "cwbl_internal.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _constant(text, name):
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def _ternary_chain(text, name, consts):
    """The body `return level <= A ? x : level <= B ? y : ... : z;` of a constexpr function of
    the header as a Python function of the level."""
    body = re.search(rf"constexpr int {name}\(int level\) \{{\s*return ([^;]+);", text).group(1)
    *conds, last = [p.strip() for p in body.split(":")]
    steps = []
    for cnd in conds:
        m = re.fullmatch(r"level <= (\w+) \? (\d+)", cnd)
        assert m, cnd
        steps.append((int(consts.get(m.group(1), m.group(1))), int(m.group(2))))

    def f(level):
        for bound, value in steps:
            if level <= bound:
                return value
        return int(last)
    return f


def test_level_helpers_equal_the_header():
    text = _header()
    consts = {n: _constant(text, n) for n in ("kQuadLevels", "kQuadLevels31")}
    assert (QUAD_LEVELS, QUAD_LEVELS_31) == (consts["kQuadLevels"], consts["kQuadLevels31"])
    rounds = _ternary_chain(text, "quad_rounds", consts)
    passes = _ternary_chain(text, "quad_passes", consts)
    for level in range(1, QUAD_LEVELS + 1):
        assert quad_rounds(level) == rounds(level), level
        assert quad_passes(level) == passes(level), level
    assert sorted({rounds(v) for v in range(1, 25)}) == [2, 3, 4, 8]
    # the decade loop: level L covers ratios in (10^(L-1), 10^L], the last level everything above
    assert [quad_level(r) for r in (0.5, 1.0, 10.0, 10.000001, 999.0, 1e12, 1.0001e12)] == \
        [1, 1, 1, 2, 3, 12, 13]
    assert quad_level(1e23 * 1.001) == quad_level(1e30) == QUAD_LEVELS
    assert near_decade(1e12 * (1 + 5e-10)) and not near_decade(1e12 * (1 + 5e-9))
    # the kernels' own statement of the loop, in every solve kernel that chooses a rule
    src = os.path.join(REPO, "cwbnwp-letkf_amd", "csrc")
    n = 0
    for name in sorted(os.listdir(src)):
        if name.startswith("cwbl_tq") and name.endswith(".hip"):
            with open(os.path.join(src, name)) as f:
                code = f.read()
            if "dec < ratio" in code:
                n += 1
                assert re.search(r"int level = 1;\s*double dec = 10\.0;\s*while \(level < "
                                 r"kQuadLevels && dec < ratio\) \{\s*dec \*= 10\.0;\s*\+\+level;",
                                 code), name
    assert n >= 7, n


def test_the_parametrisation_covers_every_class():
    """Across the cases: the record path R = 2, 3, 4, 8 and a mixed wave; every other k both
    pass counts and a case where they meet among neighbouring points."""
    rec = [c for c in sc.CASES if sc.on_record_path(c.k)]
    assert sorted({r for c in rec for r in c.classes}) == [2, 3, 4, 8]
    assert any(c.mixed and set(c.classes) == {4, 8} for c in rec)
    assert any(c.mixed and set(c.classes) == {3, 4} for c in rec)
    for k in (16, 64, 96, 128):
        mine = [c for c in sc.CASES if c.k == k]
        assert {(1,), (2,), (1, 2)} <= {c.classes for c in mine}, k
        assert any(c.mixed for c in mine), k


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_input_conditions(c):
    w = sc.workload(c)
    assert w.points == 720
    assert sc.means_exact(w)
    ev = sc.evaluate(c, floor=True)
    assert np.count_nonzero(ev.levels) == w.points           # every point has obs
    assert ev.near.sum() == 0
    assert sc.classes_present(c, ev.levels) == sorted(c.classes)
    mixed = sc.mixed_fours(c, ev.levels)
    assert (mixed > 0) == c.mixed, mixed
    if c.e <= -16:
        assert ev.levels.max() >= 13
    floor = increment_rel_rms(ev.truth, ev.truth_rev, w.var)
    u, n = np.unique(ev.levels, return_counts=True)
    print(f"{sc.case_id(c)}: levels {dict(zip(u.tolist(), n.tolist()))}, {mixed} mixed fours, "
          f"fp64 floor {floor:.3e}, bound {c.tol} x INCR_TOL")
    if c.tol == 1:
        assert floor <= sc.INCR_TOL / 4, floor
    else:  # the smallest multiple of INCR_TOL >= 4 x floor (10 % for another LAPACK's rounding)
        assert 4 * floor <= c.tol * sc.INCR_TOL <= 4.4 * floor + sc.INCR_TOL, floor
        assert abs(floor / sc.SPARSE_FLOORS[c.k][0] - 1) <= 0.1, floor
