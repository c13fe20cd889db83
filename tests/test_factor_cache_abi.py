"""CPU checks of the interface of the factor caches' options (CWBL_OPT_WAVE_REUSE, _BIG_REUSE,
_ROWS_REUSE; FORMS): each option's number in the C header, the Python binding and the Fortran
module, its range and default in the library source, the unchanged ABI version, and the size of
a cached factor (WaveFactor<KP>, BigFactor<96, 32>, BigFactor<128, 64>; cwbl_internal.h) against
the formula or the bound the documents state."""
import dataclasses
import os
import re
import typing

import pytest

from cwbl import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "cwbnwp-letkf_amd")
HEADER = os.path.join("include", "cwb_letkf_core.h")
DOCS = ("README.md", "DESIGN.md", HEADER)


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


@dataclasses.dataclass(frozen=True)
class Form:
    id: str
    number: int
    f90_alone: bool       # test_option_number also counts the number in the Fortran module
    declared: bool        # test_option_range...: also the State member's initialiser
    header_says: tuple    # ... and these words in the header's text of the option
    factor: typing.Optional[tuple]  # BigFactor's (KP, J0, words, bound); None: WaveFactor
    parts: typing.Optional[tuple]   # BigFactor's per-row arrays, reflectors and tail columns
    selected: typing.Optional[str]  # the regex of big_factor_words' branch

    @property
    def name(self):
        return self.id + "_reuse"

    @property
    def opt(self):
        return "CWBL_OPT_" + self.name.upper()


FORMS = (
    Form("wave", 19, f90_alone=False, declared=False, header_says=(), factor=None, parts=None,
         selected=None),
    Form("big", 21, f90_alone=True, declared=False,
         header_says=("0 (default)", "ignored at k = 97..128"), factor=(96, 32, 4977, 5040),
         parts=None, selected=None),
    Form("rows", 22, f90_alone=True, declared=True,
         header_says=("0 (default)", "ignored at", "k <= 96"), factor=(128, 64, 8705, 8768),
         parts=(640, 6112, 1953), selected=r"kp == 128 \? BigFactor<128, 64>::WORDS"),
)


def forms(*ids):
    return pytest.mark.parametrize("form", [f for f in FORMS if not ids or f.id in ids],
                                   ids=lambda f: f.id)


@forms()
def test_option_number(form):
    n = form.number
    hdr = read(REPO, HEADER)
    assert re.search(rf"\b{form.opt}\s*=\s*{n}\b", hdr)
    assert getattr(abi, "OPT_" + form.name.upper()) == n and abi.OPTIONS[form.name] == n
    f90 = read(PKG, "fortran", "letkf_core_gpu.f90")
    assert re.search(rf"parameter,\s*public\s*::\s*{form.opt}\s*=\s*{n}\b", f90)
    # the number is the option's alone
    assert sorted(abi.OPTIONS.values()).count(n) == 1
    assert len(re.findall(rf"\bCWBL_OPT_\w+\s*=\s*{n}\b", hdr)) == 1
    if form.f90_alone:
        assert len(re.findall(rf"::\s*CWBL_OPT_\w+\s*=\s*{n}\b", f90)) == 1


@forms("big", "rows")
def test_option_range_in_the_library_source(form):
    """0 and 1, as the header says; the default is 0 and cwbl_init resets it."""
    src = read(PKG, "csrc", "cwbl_abi.hip")
    case = src[src.index(f"case {form.opt}:"):]
    case = case[:case.index("return CWBL_OK;")]
    assert "range(0, 1)" in case, case
    if form.declared:
        assert re.search(rf"bool {form.name}\s*=\s*false;", src)
    assert re.search(rf"S\.{form.name}\s*=\s*false;", src)
    hdr = read(REPO, HEADER)
    text = hdr[hdr.index(form.opt):]
    text = text[:text.index("*/")]
    assert all(words in text for words in form.header_says), text


@forms()
def test_abi_version_stays(form):
    assert abi.ABI_VERSION == 2
    assert re.search(r"#define\s+CWBL_ABI_VERSION\s+2\b", read(REPO, HEADER))


def _const(body, name, env):
    m = re.search(rf"\b{name}\s*=\s*([^;]+);", body)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[A-Za-z0-9_\s()*/+\-]+", expr), expr
    return eval(expr.replace("/", "//"), dict(env))


def _wave_factor_words():
    """KP (KP - 1) / 2 + 5 KP fp64 words per point: 10.9, 14.6 and 18.7 KB at KP = 48, 56, 64,
    as the header, README and DESIGN.md state."""
    src = read(PKG, "csrc", "cwbl_internal.h")
    body = src[src.index("struct WaveFactor"):]
    body = body[:body.index("};")]
    m = re.search(r"WORDS\s*=\s*([^;]+);", body)
    assert m, body
    expr = m.group(1)
    assert re.fullmatch(r"[KP0-9\s()*/+\-]+", expr), expr
    col = re.search(r"COL\s*=\s*([^;]+);", body).group(1)
    for kp, kb in ((48, 10.9), (56, 14.6), (64, 18.7)):
        words = eval(expr.replace("/", "//"), {"KP": kp})
        assert words == kp * (kp - 1) // 2 + 5 * kp
        assert round(words * 8 / 1e3, 1) == kb, (kp, words)
        # the five per-row arrays come first, the packed columns after them
        assert eval(col.replace("/", "//"), {"KP": kp}) == 5 * kp
    for doc in DOCS:
        text = read(REPO, doc)
        assert re.search(r"KP\s*\(KP\s*[-−]\s*1\)\s*/\s*2\s*\+\s*5\s*KP", text), doc


def _big_factor_words(form):
    """BigFactor<KP, J0>: five per-row arrays, the hand-off kernel's J0 reflectors (rows
    j + 1 .. KP-1), the tail's 62 columns (rows j + 2 .. KP-1): 4977 fp64 words at <96, 32> and
    8705 (640 + 6112 + 1953) at <128, 64>, within the bound KP (KP - 1) / 2 + 5 KP = 5040
    (40 320 B) and 8768 that the header, README and DESIGN.md state."""
    kp, j0, want_words, want_bound = form.factor
    src = read(PKG, "csrc", "cwbl_internal.h")
    body = src[src.index("struct BigFactor"):]
    body = body[:body.index("};")]
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
    if form.parts:
        assert (f_hv(0), f_hv(j0) - f_hv(0), f_bt(62) - f_bt(0)) == form.parts
    assert re.search(r"WORDS\s*=\s*bt\(KT - 2\);", body)
    words = f_bt(env["KT"] - 2)
    bound = kp * (kp - 1) // 2 + 5 * kp
    assert words == want_words and bound == want_bound and words <= bound
    assert re.search(rf"static_assert\(BigFactor<{kp}, {j0}>::WORDS <= {kp} \* {kp - 1} / 2 "
                     rf"\+ 5 \* {kp}", src)
    if form.selected:
        assert re.search(form.selected, src)
    for doc in DOCS:
        text = read(REPO, doc)
        assert form.opt in text and str(want_words) in text, doc


@forms()
def test_factor_words(form):
    """The exact words of the form's factor (_wave_factor_words, _big_factor_words)."""
    if form.factor is None:
        _wave_factor_words()
    else:
        _big_factor_words(form)
