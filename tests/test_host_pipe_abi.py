"""CPU checks of CWBL_OPT_HOST_PIPE's interface: the option's number in the C header, in
abi.OPTIONS and in the Fortran module (and that no other option has it), the layout of
cwbl_transfer_info_t against the C compiler (the method of test_abi.test_struct_layouts_match_c),
the reason codes, the exported symbol, the Fortran binding, and the unchanged ABI version."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
F90 = os.path.join(REPO, "cwbnwp-letkf_amd", "fortran", "letkf_core_gpu.f90")
LIB = abi.default_library_path()


def test_option_number_is_20_everywhere_and_unique():
    hdr, f90 = open(HEADER).read(), open(F90).read()
    assert re.search(r"\bCWBL_OPT_HOST_PIPE\s*=\s*20\b", hdr)
    assert abi.OPT_HOST_PIPE == 20 and abi.OPTIONS["host_pipe"] == 20
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_HOST_PIPE\s*=\s*20\b", f90)
    assert sorted(abi.OPTIONS.values()).count(20) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*20\b", hdr)) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*20\b", f90)) == 1
    # every option of the header has its number in abi.OPTIONS, and those the Fortran module
    # declares have the header's number
    # (the enumerators: at the start of a line; the comments name options mid-line)
    opts = {name: int(num) for name, num in re.findall(r"^\s*CWBL_OPT_(\w+) = (\d+)", hdr, re.M)}
    assert len(opts) == len(abi.OPTIONS) and len(set(opts.values())) == len(opts)
    for name, num in opts.items():
        assert abi.OPTIONS[name.lower()] == num, name
    for name, num in re.findall(r"public\s*::\s*CWBL_OPT_(\w+)\s*=\s*(\d+)", f90):
        assert opts[name] == int(num), name


def test_abi_version_is_unchanged():
    assert "#define CWBL_ABI_VERSION 2" in open(HEADER).read() and abi.ABI_VERSION == 2


def test_reason_numbers_match_the_header_and_fortran():
    hdr, f90 = open(HEADER).read(), open(F90).read()
    for name in ("PIPED", "REASON_OFF", "REASON_REGION", "REASON_REGISTER", "REASON_BOUNCE"):
        m = re.search(rf"CWBL_TRANSFER_{name} = (\d+)", hdr)
        assert m and int(m.group(1)) == getattr(abi, f"TRANSFER_{name}"), name
        assert re.search(rf"\bCWBL_TRANSFER_{name}\s*=\s*{m.group(1)}\b", f90), name


def test_transfer_info_layout_matches_c():
    py = abi.TransferInfo
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("size %zu\\n", sizeof(cwbl_transfer_info_t));',
             'printf("column %zu\\n", sizeof(cwbl_column_info_t));',
             'printf("stats %zu\\n", sizeof(cwbl_stats));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwbl_transfer_info_t, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got["size"]) == C.sizeof(py) == 64
    assert int(got["column"]) == C.sizeof(abi.ColumnInfo) == 32  # as it was
    assert int(got["stats"]) == C.sizeof(abi.Stats)              # as it was
    for fname, _ in py._fields_:
        assert int(got[fname]) == getattr(py, fname).offset, fname
    # the header's fields, in its order
    body = re.search(r"typedef struct cwbl_transfer_info_t \{(.*?)\} cwbl_transfer_info_t;",
                     open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in py._fields_]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "cwbnwp-letkf_amd"), "-j4", "all"],
                       check=True, capture_output=True)
    return abi.load_library(LIB)


def test_library_exports_the_symbol_and_needs_init(lib):
    assert re.search(r"int\s+cwbl_transfer_info\(cwbl_transfer_info_t \*out\);",
                     open(HEADER).read())
    assert "cwbl_transfer_info" in abi.EXPORTS
    assert hasattr(lib, "cwbl_transfer_info")
    assert lib.cwbl_transfer_info(C.byref(abi.TransferInfo())) == 2  # CWBL_ERR_STATE
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_set_option(abi.OPT_HOST_PIPE, 1) == 2


def test_fortran_binding_declares_the_transfer_interface():
    src = open(F90).read()
    assert "bind(C, name='cwbl_transfer_info')" in src
    assert "type, bind(C), public :: cwbl_transfer_info_t" in src
    # the derived type's components, in the header's order and kinds
    body = re.search(r"public :: cwbl_transfer_info_t.*?\n(.*?)end type cwbl_transfer_info_t",
                     src, re.S).group(1)
    comps = []
    for kind, names in re.findall(r"integer\((c_int|c_long_long)\)\s*::\s*(.*)", body):
        comps += [(n.strip(), kind) for n in names.split(",")]
    want = [(f, "c_int" if t is C.c_int else "c_long_long") for f, t in abi.TransferInfo._fields_]
    assert comps == want
