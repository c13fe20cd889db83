"""Resource checks of the factor cache's kernels of the one-wavefront path (CPU: compiles
cwbl_tq_wave.hip to gfx950 assembly with test_isa.py's flags and reads the kernels' metadata
only): fill_tq_wave_kernel<KP> and solve_tq_wave_factor_kernel<KP> at KP = 48, 56, 64 are free
of scratch, keep the waves per SIMD of TqOccupancy<KP> (3 at 48, 2 above: at most 170 and 256
VGPRs; the hit holds a factor's columns in registers) and use no more LDS than
solve_tq_kernel<KP>'s TqSmem<KP>."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, needs_hipcc
from test_isa_tq_multi import LDS, waves

KERNELS = {"19fill_tq_wave_kernel": "fill_tq_wave_kernel",
           "27solve_tq_wave_factor_kernel": "solve_tq_wave_factor_kernel"}


@needs_hipcc
def test_wave_reuse_budgets(tmp_path):
    src = os.path.join(SRC, "cwbl_tq_wave.hip")
    asm = tmp_path / "tq_wave.s"
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
        m = re.match(r"_ZN4cwbl(\d+[a-z_0-9]+?kernel)ILi(\d+)EEEv", name)
        assert m and m.group(1) in KERNELS, name
        field = lambda f: int(re.search(rf"^\s*\.{f}:\s+(\d+)", rec, re.M).group(1))
        seen[(KERNELS[m.group(1)], int(m.group(2)))] = (
            field("vgpr_count"), field("group_segment_fixed_size"),
            field("private_segment_fixed_size"))
    assert sorted(seen) == [(n, kp) for n in sorted(KERNELS.values()) for kp in (48, 56, 64)], \
        sorted(seen)
    for (name, kp), (vgpr, lds, scratch) in sorted(seen.items()):
        print(f"{name}<{kp}>: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch")
        assert scratch == 0, (name, kp, scratch)
        assert vgpr <= 512 // waves(kp), (name, kp, vgpr)
        assert lds <= LDS[kp], (name, kp, lds)
