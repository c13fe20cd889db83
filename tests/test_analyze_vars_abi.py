"""CPU checks of the cwbl_analyze_vars additions: the declaration in the header, the Python and
Fortran bindings, the state error before cwbl_init, and namelist.var_groups, the host's
grouping of var_update into calls."""
import copy
import ctypes as C
import os
import re
import subprocess

import pytest

from cwbl import abi, namelist
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
LIB = abi.default_library_path()
NML = os.path.join(REPO, "tests", "golden", "namelist", "input.nml")


def test_header_declares_the_entry_point():
    src = open(HEADER).read()
    assert re.search(r"#define\s+CWBL_MAX_GROUP_VARS\s+8\b", src)
    assert re.search(r"\bint\s+cwbl_analyze_vars\s*\(\s*int\s+nvar\s*,\s*const\s+cwbl_var_params\s*\*",
                     src)
    assert "#define CWBL_ABI_VERSION 2" in src  # an added entry point, no struct changed


def test_python_binding():
    assert "cwbl_analyze_vars" in abi.EXPORTS
    assert abi.ABI_VERSION == 2
    assert abi.MAX_GROUP_VARS == 8
    assert callable(abi.Core.analyze_vars)


def test_fortran_binding_declares_the_interface():
    src = open(os.path.join(REPO, "cwbnwp-letkf_amd", "fortran", "letkf_core_gpu.f90")).read()
    assert "bind(C, name='cwbl_analyze_vars')" in src
    assert "CWBL_MAX_GROUP_VARS = 8" in src
    public = src[src.index("public :: cwbl_init"):src.index("\n    interface\n")]
    assert re.search(r"\bcwbl_analyze_vars\b", public)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "cwbnwp-letkf_amd"), "-j4", "all"],
                       check=True, capture_output=True)
    return abi.load_library(LIB)


def test_entry_point_needs_init(lib):
    """Without a device, or before cwbl_init: an error, no crash (null arguments included)."""
    vp, slab, st = abi.VarParams(), abi.Slab(), abi.Stats()
    assert lib.cwbl_analyze_vars(1, C.byref(vp), C.byref(slab), C.byref(st)) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_analyze_vars(0, None, None, None) == 2


def test_var_groups_of_the_golden_namelist():
    cfg = namelist.read_namelist(NML)
    groups = namelist.var_groups(cfg)
    assert groups == [[0], [1], [2], [3, 4], [5, 6, 7, 8, 9, 10, 11, 12], [13], [14], [15]]
    names = namelist.var_names(cfg)
    assert [names[i] for i in groups[3]] == ["T", "QVAPOR"]
    assert [names[i] for i in groups[4]] == ["QRAIN", "QSNOW", "QGRAUP", "QHAIL", "QNRAIN",
                                             "QNSNOW", "QNGRAUPEL", "QNHAIL"]
    assert all(len(g) <= abi.MAX_GROUP_VARS for g in groups)
    # a group's members have equal key fields, as the library's group rule asks
    for g in groups:
        vps = [namelist.var_params(cfg, i + 1) for i in g]
        for vp in vps[1:]:
            assert vp.multi_infl == vps[0].multi_infl
            assert bytes(vp.gts) == bytes(vps[0].gts) and bytes(vp.radar) == bytes(vps[0].radar)


def test_var_groups_split():
    cfg = namelist.read_namelist(NML)
    one = copy.deepcopy(cfg)
    one["inflation"]["multi_infl"][8] = 1.2  # QHAIL, inside the group of eight
    assert namelist.var_groups(one)[4:7] == [[5, 6, 7], [8], [9, 10, 11, 12]]
    loc = copy.deepcopy(cfg)
    loc["observations"]["radar_nml"]["dbz"]["hclr"][6] = 9.0  # QSNOW's dbz localisation
    assert namelist.var_groups(loc)[4:7] == [[5], [6], [7, 8, 9, 10, 11, 12]]
    # the grid tag: everything on one grid lets T .. QNHAIL's keys alone decide; a tag per
    # variable splits every group
    assert namelist.var_groups(cfg, grid_of=lambda name: name) == [[i] for i in range(16)]
    assert namelist.var_groups(cfg, grid_of={"QVAPOR": "other"})[3:5] == [[3], [4]]


def test_var_groups_split_at_the_group_limit(monkeypatch):
    """A run longer than the call's limit is split in var_update order."""
    cfg = namelist.read_namelist(NML)
    monkeypatch.setattr(abi, "MAX_GROUP_VARS", 3)
    groups = namelist.var_groups(cfg)
    assert groups[3:7] == [[3, 4], [5, 6, 7], [8, 9, 10], [11, 12]]
    assert [i for g in groups for i in g] == list(range(16))
