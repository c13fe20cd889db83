"""Resource checks of the group kernels of the hand-off path (CPU: compiles
cwbl_tq_rows_multi.hip, cwbl_tq_big_multi.hip and cwbl_tq_tail_multi.hip to gfx950 assembly
with test_isa.py's flags and reads the kernels' metadata only).  Every instantiation (two
heads and two tails by NV = 2, 4, 8) is free of scratch, and

- solve_tq_rows_multi_kernel<128, 64, NV> keeps solve_tq_rows_kernel's two workgroups per CU:
  at most 256 VGPRs and 80 KB of LDS;
- solve_tq_big_multi_kernel<96, 32, NV> keeps solve_tq_big_kernel<96, false, 32>'s three
  workgroups per CU: at most 168 VGPRs and 160 KB / 3 of LDS;
- solve_tqb_tail_multi_kernel<96, 32, NV> keeps solve_tqb_tail_kernel<96, 32, 2>'s two waves
  per SIMD: at most 256 VGPRs, and LDS for eight one-wave workgroups per CU;
- solve_tqb_tail_multi_kernel<128, 64, NV> runs at two waves per SIMD (at most 256 VGPRs, LDS
  for eight workgroups per CU), not the three of solve_tqb_tail_kernel<128, 64, 3>, which
  takes its 168 VGPRs with 140 B of scratch per lane: without scratch the group form does not
  fit them.
"""
import os
import re
import subprocess

import pytest

from test_isa import HIPCC, SRC, needs_hipcc

LDS_CU = 160 * 1024
# kernel -> (VGPRs for its waves per SIMD, LDS for its workgroups per CU)
BUDGET = {
    ("solve_tq_rows_multi_kernel", 128, 64): (512 // 2, 80 * 1024),
    ("solve_tq_big_multi_kernel", 96, 32): (512 // 3, LDS_CU // 3),
    ("solve_tqb_tail_multi_kernel", 96, 32): (512 // 2, LDS_CU // 8),
    ("solve_tqb_tail_multi_kernel", 128, 64): (512 // 2, LDS_CU // 8),
}
SOURCES = {"cwbl_tq_rows_multi.hip": ["solve_tq_rows_multi_kernel"],
           "cwbl_tq_big_multi.hip": ["solve_tq_big_multi_kernel"],
           "cwbl_tq_tail_multi.hip": ["solve_tqb_tail_multi_kernel"]}


@needs_hipcc
@pytest.mark.parametrize("source", sorted(SOURCES))
def test_big_multi_budgets(source, tmp_path):
    src = os.path.join(SRC, source)
    assert os.path.exists(src), src
    asm = tmp_path / (source + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    seen = {}
    # one metadata record per kernel: its fields in alphabetical order, .name among them
    for rec in text.split("- .agpr_count:")[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", rec, re.M).group(1)
        m = re.match(r"_ZN4cwbl\d+(solve_\w+_multi_kernel)ILi(\d+)ELi(\d+)ELi(\d+)EEEv", name)
        assert m, name
        field = lambda f: int(re.search(rf"^\s*\.{f}:\s+(\d+)", rec, re.M).group(1))
        seen[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = (
            field("vgpr_count"), field("group_segment_fixed_size"),
            field("private_segment_fixed_size"))
    want = [key + (nv,) for key in sorted(BUDGET) if key[0] in SOURCES[source]
            for nv in (2, 4, 8)]
    assert sorted(seen) == want, sorted(seen)
    for key, (vgpr, lds, scratch) in sorted(seen.items()):
        name, kp, j0, nv = key
        print(f"{name}<{kp}, {j0}, {nv}>: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch")
        max_vgpr, max_lds = BUDGET[key[:3]]
        assert scratch == 0, (key, scratch)
        assert vgpr <= max_vgpr, (key, vgpr)
        assert lds <= max_lds, (key, lds)
