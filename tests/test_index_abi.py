"""CPU checks of the search-index additions to the C ABI: the option number, the layouts of
cwbl_bin_grid and cwbl_prep_info_t against the C compiler (the method of
test_abi.test_struct_layouts_match_c), and the state error of the two entry points before
cwbl_init."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
LIB = abi.default_library_path()

STRUCTS = {"cwbl_bin_grid": abi.BinGrid, "cwbl_prep_info_t": abi.PrepInfo}


def test_index_option_number():
    assert abi.OPTIONS["index"] == 13
    assert abi.OPT_INDEX == 13
    src = open(HEADER).read()
    assert "CWBL_OPT_INDEX = 13" in src
    assert "#define CWBL_ABI_VERSION 2" in src and abi.ABI_VERSION == 2


def test_index_struct_layouts_match_c():
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    for cname, py in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "cwbnwp-letkf_amd"), "-j4", "all"],
                       check=True, capture_output=True)
    return abi.load_library(LIB)


def test_index_entry_points_need_init(lib):
    """No cwbl_init: both entry points report the state error, nothing runs."""
    grid = abi.BinGrid()
    assert lib.cwbl_bin_index(0, None, 10.0, -1.0, 2, C.byref(grid), 0, None, None,
                              abi.MEM_HOST) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_prep_info(C.byref(abi.PrepInfo())) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_set_option(abi.OPT_INDEX, 1) == 2


def test_fortran_binding_declares_the_index_interface():
    src = open(os.path.join(REPO, "cwbnwp-letkf_amd", "fortran", "letkf_core_gpu.f90")).read()
    assert "CWBL_OPT_INDEX = 13" in src
    for name in ("cwbl_bin_index", "cwbl_prep_info"):
        assert f"bind(C, name='{name}')" in src
