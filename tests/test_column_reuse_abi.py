"""CPU checks of the interface of CWBL_OPT_COLUMN_REUSE: the option's number once each in the C
header, the Python binding and the Fortran module; its range, default and reset in the library
source; the unchanged ABI version; and cwbl_column_reuse_info_t in C (against the compiler, the
method of test_column_factor_abi.py), Python and Fortran, with its entry point among the exports.
cwbl_column_info_t stays as it is (test_column_factor_abi.py pins its 32 bytes)."""
import ctypes as C
import os
import re
import subprocess

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
PKG = os.path.join(REPO, "cwbnwp-letkf_amd")
F90 = os.path.join(PKG, "fortran", "letkf_core_gpu.f90")
FIELDS = ["columns_reused", "columns_filled", "batches_reused", "bytes_held", "ms_compare",
          "form", "reserved"]


def read(path):
    with open(path) as f:
        return f.read()


def test_option_number():
    hdr, f90 = read(HEADER), read(F90)
    assert re.search(r"\bCWBL_OPT_COLUMN_REUSE\s*=\s*24\b", hdr)
    assert abi.OPT_COLUMN_REUSE == 24 and abi.OPTIONS["column_reuse"] == 24
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_COLUMN_REUSE\s*=\s*24\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(24) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*24\b", hdr)) == 1
    assert len(re.findall(r"::\s*CWBL_OPT_\w+\s*=\s*24\b", f90)) == 1
    # every option of the header has its number in abi.OPTIONS
    opts = dict(re.findall(r"^\s*CWBL_OPT_(\w+)\s*=\s*(\d+)", hdr, re.M))
    assert len(opts) == len(abi.OPTIONS)
    for name, num in opts.items():
        assert abi.OPTIONS[name.lower()] == int(num), name


def test_abi_version_stays():
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(HEADER))


def test_option_range_default_and_reset_in_the_library_source():
    """A budget in MiB, 0 .. 2^24; the default is 0, cwbl_init resets it, 0 releases the cache,
    and like every option that decides what is cached it starts a new generation."""
    src = read(os.path.join(PKG, "csrc", "cwbl_abi.hip"))
    assert re.search(r"size_t column_reuse\s*=\s*0;", src)
    assert re.search(r"S\.column_reuse\s*=\s*0;", src)
    block = src[src.index("case CWBL_OPT_COLUMN_REUSE:"):]
    block = block[:block.index("return CWBL_OK;")]
    assert "range(0, 1LL << 24)" in block and "<< 20" in block and "S.ccache.release()" in block
    # the case stands behind the generation's increment, not among the options that keep it
    assert src.index("++S.gen;  // options change") < src.index("case CWBL_OPT_COLUMN_REUSE:")
    text = read(HEADER)
    text = text[text.index("CWBL_OPT_COLUMN_REUSE = 24"):]
    text = text[:text.index("*/")]
    for words in ("0 = off", "MiB", "nz = 1", "k <= 16", "k = 97..128", "no error",
                  "CWBL_OPT_SPLIT40 = 0", "CWBL_OPT_SOLVER = 1", "CWBL_OPT_BIG_PATH = 0",
                  "group calls"):
        assert words in text, words


def test_column_reuse_info_layout(tmp_path):
    py = abi.ColumnReuseInfo
    assert [n for n, _ in py._fields_] == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){",
             'printf("size %zu\\n", sizeof(cwbl_column_reuse_info_t));']
    for n in FIELDS:
        lines.append(f'printf("{n} %zu\\n", offsetof(cwbl_column_reuse_info_t, {n}));')
    for i, n in enumerate(("NONE", "RECORDS", "WAVE", "BIG")):
        lines.append(f'printf("form_{n} %d\\n", CWBL_COLUMN_FORM_{n} == {i});')
    lines.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.split() for line in out.split("\n") if line)
    assert int(got["size"]) == C.sizeof(py) == 48
    for n in FIELDS:
        assert int(got[n]) == getattr(py, n).offset, n
    for n in ("NONE", "RECORDS", "WAVE", "BIG"):
        assert got["form_" + n] == "1", n
    assert (abi.COLUMN_FORM_NONE, abi.COLUMN_FORM_RECORDS, abi.COLUMN_FORM_WAVE,
            abi.COLUMN_FORM_BIG) == (0, 1, 2, 3)
    assert "reserved" not in py().as_dict() and "form" in py().as_dict()


def test_entry_point_is_declared_bound_and_exported():
    assert "cwbl_column_reuse_info" in abi.EXPORTS
    assert re.search(r"int\s+cwbl_column_reuse_info\(cwbl_column_reuse_info_t \*out\);",
                     read(HEADER))
    assert hasattr(abi.Core, "column_reuse_info")
    src = read(os.path.join(PKG, "csrc", "cwbl_abi.hip"))
    assert "int cwbl_column_reuse_info(cwbl_column_reuse_info_t *out)" in src


def test_fortran_type_and_interface():
    f90 = read(F90)
    body = f90[f90.index("type, bind(C), public :: cwbl_column_reuse_info_t"):]
    body = body[:body.index("end type cwbl_column_reuse_info_t")]
    assert re.search(r"integer\(c_long_long\)\s*::\s*columns_reused, columns_filled, "
                     r"batches_reused, bytes_held\b", body), body
    assert re.search(r"real\(c_double\)\s*::\s*ms_compare\b", body), body
    assert re.search(r"integer\(c_int\)\s*::\s*form, reserved\b", body), body
    assert re.search(r"bind\(C, name='cwbl_column_reuse_info'\)", f90)
    public = f90[f90.index("public :: cwbl_init"):]
    assert "cwbl_column_reuse_info" in public[:public.index("cwbl_check")]
    for i, n in enumerate(("NONE", "RECORDS", "WAVE", "BIG")):
        assert re.search(rf"::\s*CWBL_COLUMN_FORM_{n}\s*=\s*{i}\b", f90), n
