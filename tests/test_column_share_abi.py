"""CPU checks of the column-share additions (CWBL_OPT_COLUMN_SHARE): the option numbers, the
layout of cwbl_column_info_t against the C compiler (the method of
test_abi.test_struct_layouts_match_c), the exported symbol, the Fortran binding, and
namelist.column_shared_vars, the host-side mirror of the library's eligibility rule."""
import copy
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from cwbl import abi, namelist
from helpers import GOLDEN, REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
LIB = abi.default_library_path()
NML = os.path.join(GOLDEN, "namelist", "input.nml")


def test_option_numbers_and_abi_version():
    src = open(HEADER).read()
    assert "CWBL_OPT_COLUMN_SHARE = 15" in src
    assert "CWBL_OPT_COLUMN_LEVELS = 16" in src
    assert re.search(r"int\s+cwbl_column_info\(cwbl_column_info_t \*out\);", src)
    assert "#define CWBL_ABI_VERSION 2" in src and abi.ABI_VERSION == 2
    assert abi.OPTIONS["column_share"] == abi.OPT_COLUMN_SHARE == 15
    assert abi.OPTIONS["column_levels"] == abi.OPT_COLUMN_LEVELS == 16
    assert "cwbl_column_info" in abi.EXPORTS


def test_reason_numbers_match_the_header():
    src = open(HEADER).read()
    for name in ("SHARED", "REASON_OFF", "REASON_3D", "REASON_Q1", "REASON_NZ", "REASON_PATH",
                 "REASON_GROUP", "REASON_NO_TREES"):
        m = re.search(rf"CWBL_COLUMN_{name} = (\d+)", src)
        assert m and int(m.group(1)) == getattr(abi, f"COLUMN_{name}"), name


def test_column_info_layout_matches_c():
    py = abi.ColumnInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("size %zu\\n", sizeof(cwbl_column_info_t));',
             'printf("reuse %zu\\n", sizeof(cwbl_reuse_info_t));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwbl_column_info_t, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got["size"]) == C.sizeof(py) == 32
    assert int(got["reuse"]) == C.sizeof(abi.ReuseInfo) == 32  # as it was
    for fname, _ in py._fields_:
        assert int(got[fname]) == getattr(py, fname).offset, fname


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "cwbnwp-letkf_amd"), "-j4", "all"],
                       check=True, capture_output=True)
    return abi.load_library(LIB)


def test_library_exports_the_symbol_and_needs_init(lib):
    assert hasattr(lib, "cwbl_column_info")
    assert lib.cwbl_column_info(C.byref(abi.ColumnInfo())) == 2  # CWBL_ERR_STATE
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_set_option(abi.OPT_COLUMN_SHARE, 1) == 2
    assert lib.cwbl_set_option(abi.OPT_COLUMN_LEVELS, 1) == 2


def test_fortran_binding_declares_the_column_interface():
    src = open(os.path.join(REPO, "cwbnwp-letkf_amd", "fortran", "letkf_core_gpu.f90")).read()
    assert "CWBL_OPT_COLUMN_SHARE = 15" in src
    assert "CWBL_OPT_COLUMN_LEVELS = 16" in src
    assert "bind(C, name='cwbl_column_info')" in src
    assert "type, bind(C), public :: cwbl_column_info_t" in src


def test_column_shared_vars_of_the_reference_namelist():
    cfg = namelist.read_namelist(NML)
    assert namelist.column_shared_vars(cfg) == ["MU", "P", "PH"]
    assert "library's own check decides" in " ".join(namelist.column_shared_vars.__doc__.split())


def test_one_used_3d_type_takes_the_variable_out():
    cfg = namelist.read_namelist(NML)
    names = namelist.var_names(cfg)
    i = names.index("P")
    one = copy.deepcopy(cfg)
    assert one["observations"]["sound_nml"]["use_it"]
    assert one["observations"]["sound_nml"]["hclr"][i] > 0
    one["observations"]["sound_nml"]["vclr"][i] = 2.0
    assert namelist.column_shared_vars(one) == ["MU", "PH"]
    # ... but not a 3-D type that is switched off, has no radius or assimilates nothing
    off = copy.deepcopy(one)
    off["observations"]["sound_nml"]["use_it"] = False
    assert namelist.column_shared_vars(off) == ["MU", "P", "PH"]
    norad = copy.deepcopy(one)
    norad["observations"]["sound_nml"]["hclr"][i] = -1.0
    assert namelist.column_shared_vars(norad) == ["MU", "P", "PH"]
    noassim = copy.deepcopy(one)
    for v in ("u", "v", "t", "q"):
        noassim["observations"]["sound_nml"][v]["is_assim"][i] = False
    assert namelist.column_shared_vars(noassim) == ["MU", "P", "PH"]
    # a config whose only used type is 3-D returns [] for that variable
    only = copy.deepcopy(cfg)
    for g in ("synop_nml", "ships_nml", "metar_nml", "sound_nml", "gpspw_nml"):
        only["observations"][g]["use_it"] = False
    for r in only["observations"]["radar_nml"].values():
        r["use_it"] = False
    vr = only["observations"]["radar_nml"]["vr"]
    vr["use_it"] = True
    vr["hclr"][:] = 12.0
    vr["vclr"][:] = 3.0
    assert namelist.column_shared_vars(only) == []
    vr["vclr"][i] = -1.0
    assert namelist.column_shared_vars(only) == ["P"]
