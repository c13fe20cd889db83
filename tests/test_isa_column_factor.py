"""Resource checks of the level kernels of CWBL_OPT_COLUMN_FACTOR (CPU: compiles
cwbl_tq_wave_column.hip and cwbl_tq_big_column.hip to gfx950 assembly with test_isa.py's flags
and reads the kernels' metadata only, the method of test_isa_wave_reuse.py):
solve_tq_wave_factor_column_kernel<KP> at KP = 48, 56, 64 is free of scratch, keeps the waves
per SIMD of TqOccupancy<KP> (3 at 48, 2 above: at most 170 and 256 VGPRs) and uses no more LDS
than solve_tq_kernel<KP>'s TqSmem<KP>; solve_tqb_factor_column_kernel<96, 32> is free of
scratch, stays within 256 VGPRs (two waves per SIMD, the tail's launch bound) and uses no more
LDS than solve_tqb_tail_kernel<96, 32, 2>'s TailSmem<96, 32>.  Each file holds these kernels and
no other."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, needs_hipcc
from test_isa_tq_multi import LDS, waves

TAIL_LDS = 6688  # TailSmem<96, 32>: the tail's, the fill's and the hit's (profiles/twin_merge.txt)


def metadata(tmp_path, stem):
    """{mangled kernel name: (VGPRs + AGPRs, LDS bytes, scratch bytes)} of csrc/<stem>.hip."""
    asm = tmp_path / (stem + ".s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", os.path.join(SRC, stem + ".hip"), "-o",
                        str(asm)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    # one metadata record per kernel: its fields in alphabetical order, .name among them
    for rec in asm.read_text().split("- .agpr_count:")[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", rec, re.M).group(1)
        field = lambda f: int(re.search(rf"^\s*\.{f}:\s+(\d+)", rec, re.M).group(1))
        seen[name] = (field("vgpr_count") + int(rec.split()[0]),
                      field("group_segment_fixed_size"), field("private_segment_fixed_size"))
    return seen


@needs_hipcc
def test_wave_column_budgets(tmp_path):
    seen = {}
    for name, figures in metadata(tmp_path, "cwbl_tq_wave_column").items():
        m = re.match(r"_ZN4cwbl34solve_tq_wave_factor_column_kernelILi(\d+)EEEv", name)
        assert m, name
        seen[int(m.group(1))] = figures
    assert sorted(seen) == [48, 56, 64], sorted(seen)
    for kp, (vgpr, lds, scratch) in sorted(seen.items()):
        print(f"solve_tq_wave_factor_column_kernel<{kp}>: {vgpr} VGPRs, {lds} B LDS, "
              f"{scratch} B scratch")
        assert scratch == 0, (kp, scratch)
        assert vgpr <= 512 // waves(kp), (kp, vgpr)
        assert lds <= LDS[kp], (kp, lds)


@needs_hipcc
def test_big_column_budgets(tmp_path):
    seen = metadata(tmp_path, "cwbl_tq_big_column")
    assert len(seen) == 1, sorted(seen)
    (name, (vgpr, lds, scratch)), = seen.items()
    assert re.match(r"_ZN4cwbl30solve_tqb_factor_column_kernelILi96ELi32EEEv", name), name
    print(f"solve_tqb_factor_column_kernel<96, 32>: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch")
    assert scratch == 0, scratch
    assert vgpr <= 512 // 2, vgpr
    assert lds <= TAIL_LDS, lds
