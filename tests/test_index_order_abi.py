"""CPU checks of the interface of CWBL_OPT_INDEX_ORDER: the option's number once each in the C
header, the Python binding and the Fortran module; every option of the header in abi.OPTIONS;
its range, default and reset in the library source, with its case behind the generation's
increment; CWBL_OPT_INDEX's unchanged range; the unchanged ABI version; the sizes of the
existing info structs and the layout of cwbl_index_info_t against the compiler (the method of
test_index_abi.py); the two new entry points in every layer and their state error before
cwbl_init; and the documents that describe the option."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cwbl import abi
from helpers import REPO

HEADER = os.path.join(REPO, "include", "cwb_letkf_core.h")
PKG = os.path.join(REPO, "cwbnwp-letkf_amd")
F90 = os.path.join(PKG, "fortran", "letkf_core_gpu.f90")
LIB = abi.default_library_path()

#: the info structs from before this option and their sizes, which stay
EXISTING = {"cwbl_prep_info_t": (abi.PrepInfo, 48), "cwbl_reuse_info_t": (abi.ReuseInfo, 32),
            "cwbl_column_info_t": (abi.ColumnInfo, 32),
            "cwbl_column_reuse_info_t": (abi.ColumnReuseInfo, 48),
            "cwbl_transfer_info_t": (abi.TransferInfo, 64), "cwbl_bin_grid": (abi.BinGrid, 32),
            "cwbl_stats": (abi.Stats, 112)}


def read(path):
    with open(path) as f:
        return f.read()


def test_option_number():
    hdr, f90 = read(HEADER), read(F90)
    assert re.search(r"\bCWBL_OPT_INDEX_ORDER\s*=\s*26\b", hdr)
    assert abi.OPT_INDEX_ORDER == 26 and abi.OPTIONS["index_order"] == 26
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_INDEX_ORDER\s*=\s*26\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(26) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*26\b", hdr)) == 1
    assert len(re.findall(r"::\s*CWBL_OPT_\w+\s*=\s*26\b", f90)) == 1
    # every option of the header has its number in abi.OPTIONS, each number once
    opts = dict(re.findall(r"^\s*CWBL_OPT_(\w+)\s*=\s*(\d+)", hdr, re.M))
    assert len(opts) == len(abi.OPTIONS) == len(set(abi.OPTIONS.values()))
    for name, num in opts.items():
        assert abi.OPTIONS[name.lower()] == int(num), name


def test_abi_version_stays():
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(HEADER))


def test_option_range_default_and_reset_in_the_library_source():
    """0 or 1; the default is 0, cwbl_init resets it, and like every option that changes what is
    cached it starts a new generation.  CWBL_OPT_INDEX keeps its range."""
    src = read(os.path.join(PKG, "csrc", "cwbl_abi.hip"))
    assert re.search(r"int index_order\s*=\s*0;", src)
    init = src[src.index("int cwbl_init("):src.index("int cwbl_set_option(")]
    assert re.search(r"S\.index_order\s*=\s*0;", init)
    block = src[src.index("case CWBL_OPT_INDEX_ORDER:"):]
    block = block[:block.index("return CWBL_OK;")]
    assert "range(0, 1)" in block and "S.index_order = (int)value;" in block
    # the case stands behind the generation's increment, not among the options that keep it
    assert src.index("++S.gen;  // options change") < src.index("case CWBL_OPT_INDEX_ORDER:")
    block = src[src.index("case CWBL_OPT_INDEX:"):]
    block = block[:block.index("return CWBL_OK;")]
    assert "range(0, 1)" in block and "S.index_mode = (int)value;" in block
    # the tree cache's key holds the order: entries of order 0 and 1 never mix
    assert re.search(r"t->cell_order == S\.index_order", src)


def test_header_comment_describes_the_option():
    text = read(HEADER)
    text = text[text.index("CWBL_OPT_INDEX_ORDER = 26"):]
    text = text[:text.index("*/")]
    for words in ("CWBL_OPT_INDEX = 1", "(default", "cwbl_init resets", "cell-sorted",
                  "bit-identical", "CWBL_OPT_BIN_DIV", "ignored under CWBL_OPT_INDEX = 0",
                  "new generation", "cwbl_index_info", "cwbl_index_slots"):
        assert words in text, words


def compiled_layout(structs, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {a: int(b) for a, b in (line.split() for line in out.split("\n") if line)}


def test_existing_info_structs_keep_their_sizes(tmp_path):
    got = compiled_layout({name: py for name, (py, _) in EXISTING.items()}, tmp_path)
    for name, (py, size) in EXISTING.items():
        assert got[name] == C.sizeof(py) == size, name
        for fname, _ in py._fields_:
            assert got[f"{name}.{fname}"] == getattr(py, fname).offset, (name, fname)


def test_index_info_layout_matches_c(tmp_path):
    got = compiled_layout({"cwbl_index_info_t": abi.IndexInfo}, tmp_path)
    assert got["cwbl_index_info_t"] == C.sizeof(abi.IndexInfo) == 16
    names = [n for n, _ in abi.IndexInfo._fields_]
    assert names == ["index_mode", "cell_order", "types", "trees_composed"]
    for i, fname in enumerate(names):
        assert got[f"cwbl_index_info_t.{fname}"] == getattr(abi.IndexInfo, fname).offset == 4 * i


def test_entry_points_in_every_layer():
    hdr, f90 = read(HEADER), read(F90)
    assert re.search(r"int\s+cwbl_index_info\(cwbl_index_info_t \*out\);", hdr)
    assert re.search(r"int\s+cwbl_index_slots\(int family, int type_id, int cap, "
                     r"int \*slot_obs, int \*n\);", hdr)
    for name in ("cwbl_index_info", "cwbl_index_slots"):
        assert name in abi.EXPORTS
        assert f"bind(C, name='{name}')" in f90
        assert callable(getattr(abi.Core, name[len("cwbl_"):]))
    assert re.search(r"type, bind\(C\), public :: cwbl_index_info_t", f90)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", PKG, "-j4", "all"], check=True, capture_output=True)
    return abi.load_library(LIB)


def test_entry_points_need_init(lib):
    """No cwbl_init: the new entry points and the option report the state error."""
    n = C.c_int(0)
    assert lib.cwbl_index_info(C.byref(abi.IndexInfo())) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_index_slots(1, abi.RADAR_VR, 0, None, C.byref(n)) == 2
    assert b"cwbl_init" in lib.cwbl_last_error()
    assert lib.cwbl_set_option(abi.OPT_INDEX_ORDER, 1) == 2


def test_kernels_of_the_numbering():
    """Three new kernels beside index_fill_kernel, whose text stays: plain loads and stores, no
    atomics."""
    src = read(os.path.join(PKG, "csrc", "cwbl_index.hip"))
    for name in ("index_fill_pos_kernel", "index_rank_kernel", "index_compose_kernel"):
        body = src[src.index(f"\n{name}("):]
        body = body[:body.index("\n}\n")]
        assert "atomic" not in body and "while" not in body and "for (" not in body, name
    assert "o.w = __int_as_float(i);" in src  # index_fill_kernel's payload: the obs index


def test_documents_describe_the_option():
    for path, words in (("README.md", ("CWBL_OPT_INDEX_ORDER",)),
                        ("INTEGRATION.md", ("CWBL_OPT_INDEX_ORDER", "cwbl_index_slots")),
                        ("DESIGN.md", ("CWBL_OPT_INDEX_ORDER", "rank", "byte-identical"))):
        text = read(os.path.join(REPO, path))
        for w in words:
            assert w in text, (path, w)
