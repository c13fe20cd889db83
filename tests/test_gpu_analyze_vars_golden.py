"""GPU tests of cwbl_analyze_vars on the reference's driver cases (tests/golden/driver_*.npz):
GTS types with nvar > 1, QC and gross-error rejects, the dbz norain rules, a 2-D family,
truncated neighbour lists (driver_mixed: the k-d tree re-search inside the group's shared
search) and Gaspari-Cohn weighting with its NaN points (driver_gc_k40), as groups of three
variables.  k = 8, 10, 12, 16 run solve_tq_multi_kernel, k = 20 and 40 solve_tq40_multi_kernel
and, with split40 = 0, solve_tq_multi_kernel<24|40>.

Variable 0 is the fixture's var_in and is held to the compiled reference's var_out; variables 1
and 2 are var_in plus seeded N(0,1) noise on the same slab geometry (one set of x, y, alt
arrays, as the group rule demands) and are held to the oracle on the same obs set: both at
INCR_TOL, with NaNs at identical positions.  The group equals the per-variable calls bit for
bit, counters included.  That comparison is np.array_equal on the raw bit patterns also where
the outputs hold NaNs (driver_gc_k40: 1280 values): the group kernels evaluate the single
kernels' expressions, and on the MI355X the NaN payloads come out equal too.
"""
import ctypes as C
import types

import numpy as np
import pytest

from cwbl import abi
from helpers import DriverCase, increment_rel_rms, oracle
from test_gpu_analyze_vars import Lib, bits

pytestmark = pytest.mark.gpu

INCR_TOL = 1e-6
NAMES = ["driver_c1", "driver_q1", "driver_2d", "driver_mixed", "driver_zdr", "driver_offset",
         "driver_gc_k40"]
RECORD = {"driver_zdr": 20, "driver_offset": 40, "driver_gc_k40": 40}
PARAMS = [(n, None) for n in NAMES] + [(n, 0) for n in RECORD]


def group_of(case):
    var0 = np.ascontiguousarray(case.var_in, np.float32)
    out = [var0]
    for i in (1, 2):
        rng = np.random.default_rng(100 + i)
        out.append((var0 + rng.standard_normal(var0.shape, dtype=np.float32)).astype(np.float32))
    return out


def oracle_run(case, var):
    ref = var.copy()
    st = abi.Stats()
    ob = case.obs_set()
    slab = abi.make_slab(np.ascontiguousarray(case.x, np.float32),
                         np.ascontiguousarray(case.y, np.float32),
                         np.ascontiguousarray(case.alt, np.float32), ref, case.ix_lim, case.iy_lim)
    rc = oracle().orc_analyze_var(case.k, case.wf, case.norain, 0, C.byref(ob), C.byref(case.vp),
                                  C.byref(slab), 4, C.byref(st))
    assert rc == 0
    return ref, st


@pytest.mark.parametrize("name,split40", PARAMS,
                         ids=[n + ("" if s is None else "-split40_0") for n, s in PARAMS])
def test_driver_case_as_a_group(name, split40):
    case = DriverCase(name + ".npz")
    k = case.k
    vars_ = group_of(case)
    w = types.SimpleNamespace(k=k, x=np.ascontiguousarray(case.x, np.float32),
                              y=np.ascontiguousarray(case.y, np.float32),
                              alt=np.ascontiguousarray(case.alt, np.float32))
    obs = case.obs_set()
    lib = Lib(w, {} if split40 is None else {"split40": split40}, weight_function=case.wf,
              norain_value=case.norain, obs_set=obs)
    lim = dict(ix_lim=case.ix_lim, iy_lim=case.iy_lim)
    try:
        singles = [lib.one(v, case.vp, **lim) for v in vars_]
        lib.c.set_kernel_timing(True)
        outs, cnt = lib.group(vars_, [case.vp] * 3, **lim)
        kt = lib.c.kernel_times()
    finally:
        lib.close()
    # the fused kernel of the path, and no per-variable solve kernel
    if name in RECORD and split40 is None:
        fused, single = "solve_tq40_multi_kernel<", "solve_tq40_kernel<"
    else:
        fused, single = "solve_tq_multi_kernel<", "solve_tq_kernel<"
    ran = [n for n in kt if n.startswith(fused)]
    assert len(ran) == 1 and not [n for n in kt if n.startswith(single)], kt
    # the group against the per-variable calls: bit for bit, NaN payloads included
    for i, (out, (one, scnt)) in enumerate(zip(outs, singles)):
        assert cnt == scnt, (i, cnt, scnt)
        assert np.array_equal(np.isnan(out), np.isnan(one)), i
        assert np.array_equal(bits(out), bits(one)), i
    # variable 0 against the compiled reference's output
    touched = np.any(bits(case.var_out) != bits(vars_[0]), axis=0)
    assert cnt["solved"] == touched.sum() > 0, (cnt, touched.sum())
    rel = increment_rel_rms(outs[0], case.var_out, vars_[0])
    nan0 = int(np.isnan(outs[0]).sum())
    kinds = [("gts" if t["family"] == 0 else "radar", t["type_id"], t["nvar"]) for t in case.types]
    print(f"{name} k={k} {ran[0]}: obs types (family, id, nvar) {kinds}, weight_function "
          f"{case.wf}; solved {cnt['solved']} nobs_sum {cnt['nobs_sum']} lz_truncated "
          f"{cnt['lz_truncated']} ntrees {cnt['ntrees']}; variable 0 vs reference {rel:.3e}, "
          f"{nan0} NaN values")
    assert rel <= INCR_TOL, rel
    assert nan0 == int(np.isnan(case.var_out).sum())
    for out, var in zip(outs, vars_):  # what the reference left untouched stays as it was
        assert np.array_equal(bits(out[:, ~touched]), bits(var[:, ~touched]))
    # variables 1 and 2 against the oracle on the same obs set
    for i in (1, 2):
        ref, ost = oracle_run(case, vars_[i])
        assert cnt["solved"] == ost.solved and cnt["nobs_sum"] == ost.nobs_sum
        assert cnt["lz_truncated"] == ost.lz_truncated
        r = increment_rel_rms(outs[i], ref, vars_[i])
        print(f"  variable {i} vs oracle {r:.3e}")
        assert r <= INCR_TOL, (i, r)
        assert np.array_equal(np.isnan(outs[i]), np.isnan(ref))
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(bits(outs[i]), bits(outs[j])), (i, j)
    if name == "driver_mixed":
        assert cnt["lz_truncated"] > 0       # the group's shared search ran the tree fallback
    if name == "driver_gc_k40":
        assert nan0 > 0
