"""CPU checks of CWBL_OPT_BIG_REUSE's interface: the option's number in the C header, the
Python binding and the Fortran module, the unchanged ABI version, and the size of a cached
factor (BigFactor<96, 32>, cwbl_internal.h) against the bound the documents state."""
import os
import re

from cwbl import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "cwbnwp-letkf_amd")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_option_number():
    hdr = read(REPO, "include", "cwb_letkf_core.h")
    assert re.search(r"\bCWBL_OPT_BIG_REUSE\s*=\s*21\b", hdr)
    assert abi.OPT_BIG_REUSE == 21 and abi.OPTIONS["big_reuse"] == 21
    f90 = read(PKG, "fortran", "letkf_core_gpu.f90")
    assert re.search(r"parameter,\s*public\s*::\s*CWBL_OPT_BIG_REUSE\s*=\s*21\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(21) == 1
    assert len(re.findall(r"\bCWBL_OPT_\w+\s*=\s*21\b", hdr)) == 1
    assert len(re.findall(r"::\s*CWBL_OPT_\w+\s*=\s*21\b", f90)) == 1


def test_option_range_in_the_library_source():
    """0 and 1, as the header says; the default is 0."""
    src = read(PKG, "csrc", "cwbl_abi.hip")
    case = src[src.index("case CWBL_OPT_BIG_REUSE:"):]
    case = case[:case.index("return CWBL_OK;")]
    assert "range(0, 1)" in case, case
    assert re.search(r"S\.big_reuse\s*=\s*false;", src)
    hdr = read(REPO, "include", "cwb_letkf_core.h")
    text = hdr[hdr.index("CWBL_OPT_BIG_REUSE"):]
    text = text[:text.index("*/")]
    assert "0 (default)" in text and "ignored at k = 97..128" in text, text


def test_abi_version_stays():
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(REPO, "include", "cwb_letkf_core.h"))


def _const(body, name, env):
    m = re.search(rf"\b{name}\s*=\s*([^;]+);", body)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[A-Za-z0-9_\s()*/+\-]+", expr), expr
    return eval(expr.replace("/", "//"), dict(env))


def test_factor_words():
    """BigFactor<96, 32>: five per-row arrays, the hand-off kernel's 32 reflectors (rows
    j + 1 .. KP-1), the tail's 62 columns (rows j + 2 .. KP-1): 4977 fp64 words, within the bound
    KP (KP - 1) / 2 + 5 KP = 5040 (40 320 B) that the header, README and DESIGN.md state."""
    src = read(PKG, "csrc", "cwbl_internal.h")
    body = src[src.index("struct BigFactor"):]
    body = body[:body.index("};")]
    kp, j0 = 96, 32
    env = {"KP": kp, "J0": j0}
    env["KT"] = _const(body, "KT", env)
    assert env["KT"] == 64
    for name in ("D", "C", "U1", "TAU", "SCAL", "HV"):
        env[name] = _const(body, name, env)
    assert [env[n] for n in ("D", "C", "U1", "TAU", "SCAL", "HV")] == [i * kp for i in range(6)]
    hv = re.search(r"int hv\(int j\)\s*\{\s*return ([^;]+);", body).group(1)
    bt = re.search(r"int bt\(int jl\)\s*\{\s*return ([^;]+);", body, re.S).group(1)
    f_hv = lambda j: eval(hv.replace("/", "//"), dict(env, j=j))  # noqa: E731
    env["BT"] = f_hv(j0)
    f_bt = lambda jl: eval(bt.replace("/", "//"), dict(env, jl=jl))  # noqa: E731
    # the columns are packed: reflector j has KP - 1 - j rows, the tail's step jl KT - 2 - jl
    for j in range(j0):
        assert f_hv(j + 1) - f_hv(j) == kp - 1 - j
    for jl in range(env["KT"] - 2):
        assert f_bt(jl + 1) - f_bt(jl) == env["KT"] - 2 - jl
    assert re.search(r"WORDS\s*=\s*bt\(KT - 2\);", body)
    words = f_bt(env["KT"] - 2)
    bound = kp * (kp - 1) // 2 + 5 * kp
    assert words == 4977 and bound == 5040 and words <= bound
    assert re.search(r"static_assert\(BigFactor<96, 32>::WORDS <= 96 \* 95 / 2 \+ 5 \* 96", src)
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "cwb_letkf_core.h")):
        text = read(REPO, doc)
        assert "CWBL_OPT_BIG_REUSE" in text and "4977" in text, doc
