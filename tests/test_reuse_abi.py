"""CPU checks of the record-reuse additions to the C ABI: the option number, the layout of
cwbl_reuse_info_t against the C compiler (the method of test_abi.test_struct_layouts_match_c),
the unchanged layout of cwbl_prep_info_t, and the state error before cwbl_init."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
LIB = abi.default_library_path()


def test_record_reuse_option_number():
    assert abi.OPTIONS["record_reuse"] == 14
    assert abi.OPT_RECORD_REUSE == 14
    src = open(HEADER).read()
    assert "CWBL_OPT_RECORD_REUSE = 14" in src
    assert "#define CWBL_ABI_VERSION 2" in src and abi.ABI_VERSION == 2
    assert "cwbl_reuse_info" in abi.EXPORTS


def test_reuse_info_layout_matches_c():
    py = abi.ReuseInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("size %zu\\n", sizeof(cwbl_reuse_info_t));',
             'printf("prep %zu\\n", sizeof(cwbl_prep_info_t));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwbl_reuse_info_t, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got["size"]) == C.sizeof(py) == 32
    assert int(got["prep"]) == C.sizeof(abi.PrepInfo) == 48  # cwbl_prep_info_t is as it was
    for fname, _ in py._fields_:
        assert int(got[fname]) == getattr(py, fname).offset, fname


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "cwbnwp-letkf_amd"), "-j4", "all"],
                       check=True, capture_output=True)
    return abi.load_library(LIB)


def test_reuse_entry_points_need_init(lib):
    assert lib.cwbl_reuse_info(C.byref(abi.ReuseInfo())) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_set_option(abi.OPT_RECORD_REUSE, 0) == 2


def test_fortran_binding_declares_the_reuse_interface():
    src = open(os.path.join(REPO, "cwbnwp-letkf_amd", "fortran", "letkf_core_gpu.f90")).read()
    assert "CWBL_OPT_RECORD_REUSE = 14" in src
    assert "bind(C, name='cwbl_reuse_info')" in src
    assert "type, bind(C), public :: cwbl_reuse_info_t" in src
