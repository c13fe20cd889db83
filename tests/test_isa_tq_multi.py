"""Resource checks of solve_tq_multi_kernel<KP, NV> (CPU: compiles cwbl_tq_multi.hip to gfx950
assembly with test_isa.py's flags and reads the kernels' metadata only): every instantiation
(KP = 8 .. 64 by NV = 2, 4, 8) is free of scratch, keeps the waves per SIMD of TqOccupancy<KP>
(4 up to KP = 40, 3 at 48, 2 above: at most 128, 170, 256 VGPRs) and uses the LDS of
solve_tq_kernel<KP>'s TqSmem<KP>; only <40, 8> adds four rows of Q^T x' (1 280 B)."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, needs_hipcc

# sizeof(TqSmem<KP>), as solve_tq_kernel<KP, false> reports it (profiles/r6_resource_usage.txt)
LDS = {8: 3104, 16: 3616, 24: 6056, 32: 6688, 40: 9536, 48: 13264, 56: 17376, 64: 22016}
LDS_ROWS = {(40, 8): 4 * 40 * 8}


def waves(kp):
    return 4 if kp <= 40 else 3 if kp <= 48 else 2


@needs_hipcc
def test_tq_multi_budgets(tmp_path):
    src = os.path.join(SRC, "cwbl_tq_multi.hip")
    asm = tmp_path / "tq_multi.s"
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
        m = re.match(r"_ZN4cwbl21solve_tq_multi_kernelILi(\d+)ELi(\d+)EEEv", name)
        assert m, name
        field = lambda f: int(re.search(rf"^\s*\.{f}:\s+(\d+)", rec, re.M).group(1))
        seen[(int(m.group(1)), int(m.group(2)))] = (
            field("vgpr_count"), field("group_segment_fixed_size"),
            field("private_segment_fixed_size"))
    assert sorted(seen) == [(kp, nv) for kp in sorted(LDS) for nv in (2, 4, 8)], sorted(seen)
    for (kp, nv), (vgpr, lds, scratch) in sorted(seen.items()):
        print(f"solve_tq_multi_kernel<{kp}, {nv}>: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch")
        assert scratch == 0, (kp, nv, scratch)
        assert vgpr <= 512 // waves(kp), (kp, nv, vgpr)
        assert lds <= LDS[kp] + LDS_ROWS.get((kp, nv), 0), (kp, nv, lds)
