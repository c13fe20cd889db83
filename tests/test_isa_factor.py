"""ISA checks of the record cache's kernel pair, fill_tq40_factor_kernel and
solve_tq40_factor_kernel (CPU: compiles cwbl_tq40_fill.hip to gfx950 assembly with
test_isa_multi.py's flags): exactly one kernel of each name, each within solve_tq40_kernel's
occupancy budget (at most 256 VGPRs and 20 480 B of LDS per one-wave workgroup, no scratch), read
from the kernels' metadata, and no source hazard at their inline-asm DPP FMAs.  Resource figures
only: what the kernels compute is tests/test_gpu_factor_reuse.py's matter."""
import os
import re
import subprocess

import pytest

from test_isa import HIPCC, SRC, dpp_hazards, needs_hipcc

KERNELS = ("fill_tq40_factor_kernel", "solve_tq40_factor_kernel")


@pytest.fixture(scope="module")
def asm_text(tmp_path_factory):
    src = os.path.join(SRC, "cwbl_tq40_fill.hip")
    asm = tmp_path_factory.mktemp("isa_factor") / "tq40_fill.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm.read_text()


def metadata(text):
    """{kernel symbol: {field: int}} from the amdhsa.kernels metadata: a list item at two
    spaces of indentation opens each kernel's block, whose own fields stand at four (the
    arguments' are nested deeper)."""
    doc = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"^  - ", doc, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M)
        fields = {k: int(v) for k, v in re.findall(
            r"^    \.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)",
            block, re.M)}
        if name and len(fields) == 3:
            out[name.group(1)] = fields
    return out


@needs_hipcc
def test_one_kernel_of_each_name_within_the_budgets(asm_text):
    md = metadata(asm_text)
    assert len(md) == 2, sorted(md)
    for kernel in KERNELS:
        got = [f for n, f in md.items() if kernel in n]
        assert len(got) == 1, (kernel, sorted(md))
        f = got[0]
        print(kernel, f)
        assert f["vgpr_count"] <= 256, (kernel, f)
        assert f["group_segment_fixed_size"] <= 20480, (kernel, f)
        assert f["private_segment_fixed_size"] == 0, (kernel, f)


@needs_hipcc
def test_no_dpp_source_hazard(asm_text):
    lines = [l.strip() for l in asm_text.splitlines()
             if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    # the fill's tridiagonalisation fuses its broadcasts like solve_tq40_multi_kernel's
    assert len([l for l in lines if l.startswith("v_fmac_f64_dpp")]) > 3000
    assert dpp_hazards(lines) == []
