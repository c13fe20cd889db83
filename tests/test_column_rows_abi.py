"""CPU checks of the interface of CWBL_OPT_COLUMN_ROWS: the option's number once each in the C
header, the Python binding and the Fortran module; every option of the header in abi.OPTIONS;
its range, default and reset in the library source, with its case behind the generation's
increment; the unchanged ABI version; and the unchanged sizes of cwbl_column_info_t and
cwbl_column_reuse_info_t (against the compiler, the method of test_column_reuse_abi.py)."""
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
    assert re.search(r"\bCWBL_OPT_COLUMN_ROWS\s*=\s*25\b", hdr)
    assert abi.OPT_COLUMN_ROWS == 25 and abi.OPTIONS["column_rows"] == 25
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_COLUMN_ROWS\s*=\s*25\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(25) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*25\b", hdr)) == 1
    assert len(re.findall(r"::\s*CWBL_OPT_\w+\s*=\s*25\b", f90)) == 1
    # every option of the header has its number in abi.OPTIONS
    opts = dict(re.findall(r"^\s*CWBL_OPT_(\w+)\s*=\s*(\d+)", hdr, re.M))
    assert len(opts) == len(abi.OPTIONS)
    for name, num in opts.items():
        assert abi.OPTIONS[name.lower()] == int(num), name


def test_abi_version_stays():
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(HEADER))


def test_option_range_default_and_reset_in_the_library_source():
    """0 or 1; the default is 0, cwbl_init resets it, and like every option that decides what is
    cached it starts a new generation."""
    src = read(os.path.join(PKG, "csrc", "cwbl_abi.hip"))
    assert re.search(r"bool column_rows\s*=\s*false;", src)
    assert re.search(r"S\.column_rows\s*=\s*false;", src)
    block = src[src.index("case CWBL_OPT_COLUMN_ROWS:"):]
    block = block[:block.index("return CWBL_OK;")]
    assert "range(0, 1)" in block and "S.column_rows = value == 1;" in block
    # the case stands behind the generation's increment, not among the options that keep it
    assert src.index("++S.gen;  // options change") < src.index("case CWBL_OPT_COLUMN_ROWS:")
    # both column options read it through one predicate, at KP = 128 alone
    assert re.search(r"S\.kp == kBigSplitKP && S\.column_rows", src)
    text = read(HEADER)
    text = text[text.index("CWBL_OPT_COLUMN_ROWS = 25"):]
    text = text[:text.index("*/")]
    for words in ("KP = 128", "CWBL_OPT_COLUMN_FACTOR", "CWBL_OPT_COLUMN_REUSE", "0 (default",
                  "cwbl_init resets", "nothing on its own", "no error", "CWBL_OPT_BIG_PATH = 0",
                  "CWBL_OPT_SOLVER = 1", "group", "CWBL_OPT_ROWS_REUSE", "new generation"):
        assert words in text, words


def test_the_older_options_keep_their_words():
    """Options 23 and 24 stay pinned as ignored at k = 97..128 without the new option; their
    comments name it."""
    text = read(HEADER)
    for opt in ("CWBL_OPT_COLUMN_FACTOR = 23", "CWBL_OPT_COLUMN_REUSE = 24"):
        body = text[text.index(opt):]
        body = body[:body.index("*/")]
        assert "k = 97..128" in body and "CWBL_OPT_COLUMN_ROWS = 1" in body, opt


def test_info_struct_sizes_stay(tmp_path):
    lines = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(){",
             'printf("%zu %zu\\n", sizeof(cwbl_column_info_t), sizeof(cwbl_column_reuse_info_t));',
             "return 0;}"]
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 48]
    assert C.sizeof(abi.ColumnInfo) == 32 and C.sizeof(abi.ColumnReuseInfo) == 48
