"""CPU checks of the interface of CWBL_OPT_COLUMN_FACTOR: the option's number in the C header,
the Python binding and the Fortran module (and that no other option has it), its range and
default in the library source, the unchanged ABI version, and cwbl_column_info_t: still 32
bytes, with from_factor where `reserved` was, in C (against the compiler, the method of
test_column_share_abi.py), Python and Fortran."""
import ctypes as C
import os
import re
import subprocess

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
PKG = os.path.join(REPO, "cwbnwp-letkf_amd")
F90 = os.path.join(PKG, "fortran", "letkf_core_gpu.f90")


def read(path):
    with open(path) as f:
        return f.read()


def test_option_number():
    hdr, f90 = read(HEADER), read(F90)
    assert re.search(r"\bCWBL_OPT_COLUMN_FACTOR\s*=\s*23\b", hdr)
    assert abi.OPT_COLUMN_FACTOR == 23 and abi.OPTIONS["column_factor"] == 23
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_COLUMN_FACTOR\s*=\s*23\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(23) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*23\b", hdr)) == 1
    assert len(re.findall(r"::\s*CWBL_OPT_\w+\s*=\s*23\b", f90)) == 1
    # every option of the header has its number in abi.OPTIONS
    opts = dict(re.findall(r"^\s*CWBL_OPT_(\w+)\s*=\s*(\d+)", hdr, re.M))  # the enum's lines
    assert len(opts) == len(abi.OPTIONS)
    for name, num in opts.items():
        assert abi.OPTIONS[name.lower()] == int(num), name


def test_abi_version_stays():
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(HEADER))


def test_option_range_and_default_in_the_library_source():
    """0 and 1; the default is 0 and cwbl_init resets it; column_share keeps its range 0..2."""
    src = read(os.path.join(PKG, "csrc", "cwbl_abi.hip"))
    assert re.search(r"bool column_factor\s*=\s*false;", src)
    assert re.search(r"S\.column_factor\s*=\s*false;", src)
    block = src[src.index("option == CWBL_OPT_COLUMN_FACTOR) {"):]
    block = block[:block.index("S.column_factor = value == 1;")]
    assert "range(0, 1)" in block, block
    share = src[src.index("case CWBL_OPT_COLUMN_SHARE:"):]
    assert "range(0, 2)" in share[:share.index("return CWBL_OK;")]
    text = read(HEADER)
    text = text[text.index("CWBL_OPT_COLUMN_FACTOR = 23"):]
    text = text[:text.index("*/")]
    for words in ("0 (default)", "k = 97..128", "k <= 40", "no error"):
        assert words in text, words


def test_column_info_layout(tmp_path):
    py = abi.ColumnInfo
    names = [n for n, _ in py._fields_]
    assert names == ["shared", "reason", "columns", "levels", "levels_per_wave",
                     "chunk_launches", "from_factor"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("size %zu\\n", sizeof(cwbl_column_info_t));']
    for n in names:
        lines.append(f'printf("{n} %zu\\n", offsetof(cwbl_column_info_t, {n}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.split() for line in out.split("\n") if line)
    assert int(got["size"]) == C.sizeof(py) == 32
    for n in names:
        assert int(got[n]) == getattr(py, n).offset, n
    assert py.from_factor.offset == 28  # where `reserved` was: the last int of the 32 bytes
    assert "reserved" not in read(HEADER)[read(HEADER).index("typedef struct cwbl_column_info_t"):
                                          read(HEADER).index("} cwbl_column_info_t;")]
    assert "from_factor" in py().as_dict()


def test_fortran_type_has_from_factor():
    f90 = read(F90)
    body = f90[f90.index("type, bind(C), public :: cwbl_column_info_t"):]
    body = body[:body.index("end type cwbl_column_info_t")]
    assert re.search(r"integer\(c_int\)\s*::\s*levels, levels_per_wave, chunk_launches, "
                     r"from_factor\b", body), body
    assert "reserved" not in body
