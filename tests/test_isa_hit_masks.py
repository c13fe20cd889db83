"""ISA checks of the merged hit kernel's level from the kept info (profiles/hit_masks.txt;
solve_tq40_factor_merged_kernel, cwbl_tq40_hit_merge.hip, the LEAN flag of cwbl_tq40_factor.h).
CPU: tests/test_isa_hit_lean.py's compile line and counters.

The level of a solved point comes from the info the fill kept, and a lane without one compares
its trace with three traces the host worked out.  trace / m, the kernel's first fp64 division,
and the decade loop are gone, so the quadrature's 2 x 2 solve holds the only v_div_fixup_f64
that is left (PARENT_DIV_FIXUP - 1).  The division's expansion and the loop were about 25 v_*
instructions; the kept word's clamp, the ballot's compare and the three compares with their
selects are about 18: the kernel has fewer v_* than before (PARENT_VALU).  The trace's sum
stays in the text, behind a wave-uniform branch that only a wave with an unsolved lane takes.

Of that file's other items, the replay's unit-row and zero-row selects were not built and the
staged node sums were measured and dropped, so the v_cndmask_b32 ahead of the quadrature's
division are not fewer than the parent's: the three level selects are new there and nothing
else is, which the last test bounds.

The parent's figures are this file's counters on the commit before it.  Resource and
instruction figures only: what the kernel computes is tests/test_gpu_hit_masks.py's matter."""
import os
import subprocess

import pytest

from test_isa import HIPCC, SRC, needs_hipcc
from test_isa_factor_scalars import count, kernel_lines

KERNEL = "solve_tq40_factor_merged_kernel"
PARENT_VALU = 2643
PARENT_DIV_FIXUP = 2
PARENT_CNDMASK_BEFORE_DIV = 188  # v_cndmask_b32 ahead of the quadrature's division


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    src = os.path.join(SRC, "cwbl_tq40_hit_merge.hip")
    asm = tmp_path_factory.mktemp("isa_hit_masks") / "tq40_hit_merge.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-I", SRC,
                        "--offload-device-only", "-S", src, "-o", str(asm)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return kernel_lines(asm.read_text(), KERNEL)


@needs_hipcc
def test_fewer_valu_than_the_parent(lines):
    valu = count(lines, "v_")
    print(f"{KERNEL}: {len(lines)} instructions, {valu} VALU ({PARENT_VALU} before)")
    assert valu < PARENT_VALU, valu


@needs_hipcc
def test_the_level_needs_no_division(lines):
    div = count(lines, "v_div_fixup_f64")
    assert div == PARENT_DIV_FIXUP - 1, div
    # the one that is left is the 2 x 2 solve's: the walk's v_rcp_f64 stand before it
    at = next(i for i, l in enumerate(lines) if l.startswith("v_div_fixup_f64"))
    assert count(lines[:at], "v_rcp_f64") > 0


@needs_hipcc
def test_selects_before_the_quadratures_division(lines):
    at = next(i for i, l in enumerate(lines) if l.startswith("v_div_fixup_f64"))
    cnd = count(lines[:at], "v_cndmask_b32")
    print(f"v_cndmask_b32 ahead of the quadrature's division: {cnd} "
          f"({PARENT_CNDMASK_BEFORE_DIV} before)")
    assert cnd <= PARENT_CNDMASK_BEFORE_DIV + 4, cnd
