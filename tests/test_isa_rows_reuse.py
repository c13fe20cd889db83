"""Resource checks of the factor cache's kernels of the hand-off path at KP = 128 (CPU: compiles
cwbl_tq_rows_factor.hip to gfx950 assembly with test_isa.py's flags and reads the kernels'
metadata only): the file holds fill_tqb_tail_kernel<128, 64> and solve_tqb_factor_kernel
<128, 64> and nothing else, both are free of scratch, and each stays within what the waves per
SIMD of its launch bound allow: 512 / W registers (VGPRs and AGPRs) and a compute unit's 160 KB
of LDS over its 4 W waves."""
import os
import re
import subprocess

from test_isa import HIPCC, SRC, needs_hipcc

KERNELS = {"20fill_tqb_tail_kernel": "fill_tqb_tail_kernel",
           "23solve_tqb_factor_kernel": "solve_tqb_factor_kernel"}


def launch_bounds():
    """Waves per SIMD that each kernel's __launch_bounds__(64, W) states, from the sources."""
    with open(os.path.join(SRC, "cwbl_tq_big_factor.h")) as f:
        fill = re.search(r"__launch_bounds__\(64, (\d+)\)\s*fill_tqb_tail_kernel\(", f.read())
    with open(os.path.join(SRC, "cwbl_tq_rows_factor.hip")) as f:
        text = f.read()
    assert re.search(r"__launch_bounds__\(64, kRowsHitWaves\)\s*solve_tqb_factor_kernel<128, 64>\(",
                     text)
    hit = re.search(r"constexpr int kRowsHitWaves = (\d+);", text)
    return {"fill_tqb_tail_kernel": int(fill.group(1)),
            "solve_tqb_factor_kernel": int(hit.group(1))}


@needs_hipcc
def test_rows_reuse_budgets(tmp_path):
    src = os.path.join(SRC, "cwbl_tq_rows_factor.hip")
    asm = tmp_path / "tq_rows_factor.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    bounds = launch_bounds()
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
            field("private_segment_fixed_size"), field("max_flat_workgroup_size"))
    assert sorted(seen) == [(n, 128, 64) for n in sorted(KERNELS.values())], sorted(seen)
    for (name, kp, j0), (vgpr, agpr, lds, scratch, wg) in sorted(seen.items()):
        waves = bounds[name]
        print(f"{name}<{kp}, {j0}>: {vgpr} VGPRs, {agpr} AGPRs, {lds} B LDS, {scratch} B scratch, "
              f"{waves} waves per SIMD")
        assert wg == 64, (name, wg)
        assert scratch == 0, (name, scratch)
        assert 2 <= waves <= 3, (name, waves)
        assert vgpr + agpr <= 512 // waves, (name, vgpr, agpr, waves)
        assert lds <= 160 * 1024 // (4 * waves), (name, lds, waves)
