"""ISA checks of solve_tq40_column_kernel (CPU: compiles cwbl_tq40_column.hip to gfx950 assembly
with test_isa_multi.py's flags): the kernel keeps solve_tq40_multi_kernel's occupancy budget (at
most 256 VGPRs and 20 480 B of LDS per one-wave workgroup, no scratch), read from the kernel's
metadata, and its inline-asm DPP FMAs have no source hazard."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, dpp_hazards, needs_hipcc


@needs_hipcc
def test_tq40_column_budgets_and_no_hazard(tmp_path):
    src = os.path.join(SRC, "cwbl_tq40_column.hip")
    asm = tmp_path / "tq40_column.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    # the kernel's metadata: one kernel in the file
    assert len(re.findall(r"^\s*\.name:\s+\S*solve_tq40_column_kernel", text, re.M)) == 1
    vgpr = [int(v) for v in re.findall(r"^\s*\.vgpr_count:\s+(\d+)", text, re.M)]
    lds = [int(v) for v in re.findall(r"^\s*\.group_segment_fixed_size:\s+(\d+)", text, re.M)]
    scratch = [int(v) for v in re.findall(r"^\s*\.private_segment_fixed_size:\s+(\d+)", text, re.M)]
    assert len(vgpr) == 1 and vgpr[0] <= 256, vgpr
    assert len(lds) == 1 and lds[0] <= 20480, lds
    assert scratch == [0], scratch
    lines = [l.strip() for l in text.splitlines()
             if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    assert len([l for l in lines if l.startswith("v_fmac_f64_dpp")]) > 3000  # the broadcasts are fused
    assert dpp_hazards(lines) == []
