"""Resource checks of the merged hit kernel, solve_tq40_factor_merged_kernel
(cwbl_tq40_hit_merge.hip, CWBL_OPT_HIT_MERGE), and of the two kernels it shares its text with
(CPU: compiles for gfx950 with the Makefile's code generation flags and reads the compiler's
-Rpass-analysis=kernel-resource-usage report).  The merged kernel runs the hit kernel's block
behind a scalar prologue, so it has to fit the same budget: at most 256 VGPRs, no scratch,
19 360 B of LDS, two waves per SIMD.  The per-batch hit kernel and the fill kernel keep the
figures they had before the block moved to a header (248 and 241 VGPRs).  Resource figures
only: what the kernels compute is tests/test_gpu_hit_merge.py's matter."""
import os
import re
import subprocess

import pytest

from test_isa import HIPCC, SRC, needs_hipcc

FIELDS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
          "LDS Size [bytes/block]": "lds", "VGPRs Spill": "vgpr_spill"}


def resource_report(tmp, name):
    """{kernel symbol: {field: int}} of csrc/<name>."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-c", os.path.join(SRC, name), "-o",
                        str(tmp / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?):\s+(\d+)\s+\[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def one(report, kernel):
    got = [f for n, f in report.items() if kernel + "ILi40E" in n]
    assert len(got) == 1, (kernel, sorted(report))
    print(kernel, got[0])
    return got[0]


@needs_hipcc
def test_merged_kernel_fits_the_hit_kernels_budget(tmp_path):
    f = one(resource_report(tmp_path, "cwbl_tq40_hit_merge.hip"), "solve_tq40_factor_merged_kernel")
    assert f["vgprs"] <= 256 and f["vgpr_spill"] == 0, f
    assert f["scratch"] == 0 and f["lds"] == 19360 and f["occupancy"] == 2, f


@needs_hipcc
def test_hit_and_fill_kernels_keep_their_figures(tmp_path):
    report = resource_report(tmp_path, "cwbl_tq40_fill.hip")
    hit = one(report, "solve_tq40_factor_kernel")
    fill = one(report, "fill_tq40_factor_kernel")
    assert hit["vgprs"] == 248 and fill["vgprs"] == 241, (hit, fill)
    for f in (hit, fill):
        assert f["scratch"] == 0 and f["lds"] == 19360 and f["occupancy"] == 2, f
