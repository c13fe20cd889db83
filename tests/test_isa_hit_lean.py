"""ISA checks of the merged hit kernel's lean text (solve_tq40_factor_merged_kernel,
cwbl_tq40_hit_merge.hip, the LEAN flag of cwbl_tq40_factor.h).  CPU: compiles the file for
gfx950 with tests/test_isa_hit_merge.py's line and counts ordinary VALU opcodes in the
kernel's assembly (from its label to its s_endpgm, test_isa_factor_scalars.kernel_lines).

The kernel is bound by VALU issue, and the flag exists to take VALU instructions out that
change no operand of a floating-point expression: the back-transform's second x scal products
and unit-row selects, the per-lane skip offsets of the triangular loads, and the pointer
arithmetic of the quadrature walk.  Three checks:

 * the kernel keeps its budget (at most 256 VGPRs, no scratch, no spill, 19 360 B of LDS, two
   waves per SIMD);
 * it has at least 350 v_* instructions fewer than the kernel had before the flag (PARENT_VALU,
   counted by this file's counter on the commit before it; the static sum of the pieces is
   about 450, the slack is what the compiler gives back);
 * the stretch that holds the back-transform has lost its products and selects.  The stretch
   runs from the kernel's last v_div_fixup_f64 (the quadrature's 2 x 2 solve, the last fp64
   division) to its first v_cvt_f32_f64 (the epilogue's first analysis value): the
   back-substitution, the gather of qs / qz, d and the back-transform.  The back-transform's
   text forms 44 products x scal in phase 2 (the slots with a row below j + 1: two for
   j + 1 = 1 .. 14, one for 15 .. 30) and 24 in phase 1 (v0 and two slots for each of 8
   steps), of which the compiler can drop at most the 8 v0 ones where the prefix has no row
   below j + 1, and selects the unit row in each of the 44 slots on a lane index it cannot see
   through (two v_cndmask_b32 per 64-bit select).  Without them the stretch has at least 60
   v_mul_f64 and 88 v_cndmask_b32 fewer than PARENT_MUL and PARENT_CNDMASK.

Resource and instruction figures only: what the kernel computes is
tests/test_gpu_hit_lean.py's matter."""
import os
import subprocess

import pytest

from test_isa import HIPCC, SRC, needs_hipcc
from test_isa_factor_scalars import count, kernel_lines
from test_isa_hit_merge import one, resource_report

KERNEL = "solve_tq40_factor_merged_kernel"
# this file's counters on the kernel before the LEAN flag
PARENT_VALU = 3020
PARENT_MUL = 134      # v_mul_f64 in the back-transform's stretch
PARENT_CNDMASK = 102  # v_cndmask_b32 in it


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    src = os.path.join(SRC, "cwbl_tq40_hit_merge.hip")
    asm = tmp_path_factory.mktemp("isa_hit_lean") / "tq40_hit_merge.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return kernel_lines(asm.read_text(), KERNEL)


def back_transform_stretch(lines):
    start = max(i for i, l in enumerate(lines) if l.startswith("v_div_fixup_f64"))
    end = min(i for i, l in enumerate(lines) if l.startswith("v_cvt_f32_f64"))
    assert start < end, (start, end)
    return lines[start:end]


@needs_hipcc
def test_merged_kernel_budget(tmp_path):
    f = one(resource_report(tmp_path, "cwbl_tq40_hit_merge.hip"), KERNEL)
    assert f["vgprs"] <= 256 and f["vgpr_spill"] == 0 and f["scratch"] == 0, f
    assert f["lds"] == 19360 and f["occupancy"] == 2, f


@needs_hipcc
def test_valu_instructions_removed(lines):
    valu = count(lines, "v_")
    print(f"{KERNEL}: {len(lines)} instructions, {valu} VALU ({PARENT_VALU} before)")
    assert valu <= PARENT_VALU - 350, valu


@needs_hipcc
def test_back_transform_forms_no_reflector(lines):
    s = back_transform_stretch(lines)
    mul, cnd = count(s, "v_mul_f64"), count(s, "v_cndmask_b32")
    print(f"back-transform stretch: {len(s)} instructions, {count(s, 'v_')} VALU, {mul} v_mul_f64 "
          f"({PARENT_MUL} before), {cnd} v_cndmask_b32 ({PARENT_CNDMASK} before)")
    assert mul <= PARENT_MUL - 60, mul
    assert cnd <= PARENT_CNDMASK - 88, cnd
