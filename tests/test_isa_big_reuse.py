"""Resource checks of the factor cache's kernels of the hand-off path (CPU: compiles
cwbl_tq_big_factor.hip to gfx950 assembly with test_isa.py's flags and reads the kernels'
metadata only): fill_tqb_tail_kernel<96, 32> and solve_tqb_factor_kernel<96, 32> are free of
scratch and stay within what solve_tqb_tail_kernel<96, 32, 2>'s two waves per SIMD allow: at
most 256 VGPRs (512 per SIMD lane over two waves) and no more LDS than half of a compute unit's
160 KB over its eight waves."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, needs_hipcc

KERNELS = {"20fill_tqb_tail_kernel": "fill_tqb_tail_kernel",
           "23solve_tqb_factor_kernel": "solve_tqb_factor_kernel"}
WAVES = 2                       # per SIMD: the tail's launch bound
LDS_PER_WAVE = 160 * 1024 // (4 * WAVES)


@needs_hipcc
def test_big_reuse_budgets(tmp_path):
    src = os.path.join(SRC, "cwbl_tq_big_factor.hip")
    asm = tmp_path / "tq_big_factor.s"
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
        m = re.match(r"_ZN4cwbl(\d+[a-z_0-9]+?kernel)ILi(\d+)ELi(\d+)EEEv", name)
        assert m and m.group(1) in KERNELS, name
        field = lambda f: int(re.search(rf"^\s*\.{f}:\s+(\d+)", rec, re.M).group(1))
        seen[(KERNELS[m.group(1)], int(m.group(2)), int(m.group(3)))] = (
            field("vgpr_count"), int(rec.split()[0]), field("group_segment_fixed_size"),
            field("private_segment_fixed_size"))
    assert sorted(seen) == [(n, 96, 32) for n in sorted(KERNELS.values())], sorted(seen)
    for (name, kp, j0), (vgpr, agpr, lds, scratch) in sorted(seen.items()):
        print(f"{name}<{kp}, {j0}>: {vgpr} VGPRs, {agpr} AGPRs, {lds} B LDS, {scratch} B scratch")
        assert scratch == 0, (name, scratch)
        assert vgpr + agpr <= 512 // WAVES, (name, vgpr, agpr)
        assert lds <= LDS_PER_WAVE, (name, lds)
