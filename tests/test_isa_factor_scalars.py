"""ISA checks of the step scalars the record cache keeps beside the factor (FactorAux: beta, tau
in an entry of their own, scal at row j + 1 of the factor's column j).  CPU: compiles
cwbl_tq40_fill.hip to gfx950 assembly with test_isa_factor.py's flags.

A cache hit loads beta, tau and scal as the fill's dlarfg produced them, so
solve_tq40_factor_kernel runs no dlarfg, and it is shorter than the 6 044 instructions it had
while it recomputed them.  dlarfg is the kernels' only rsq64, one v_rsq_f64 per step.  It is
not the only source of that instruction, though: tq40_factor_solve, the text both kernels
share, takes two fp64 square roots (sqrt(m) for the quadrature's weights, sqrt(k - 1) for the
analysis), and the compiler expands each from a v_rsq_f64.  So the check is not "none" but
"those two": the hit kernel has exactly the two, and the fill kernel, which runs the same
text after its 38 steps, exactly 38 more.  fill_tq40_factor_kernel keeps the reduction it had,
fused DPP FMAs included."""
import re

from test_isa import needs_hipcc
from test_isa_factor import asm_text  # noqa: F401  (the module's fixture: one compilation)

HIT_BEFORE = 6044  # instructions of solve_tq40_factor_kernel<40> with the 38 dlarfg in it
STEPS = 38         # Householder steps of KP = 40: one dlarfg each
SQRTS = 2          # fp64 square roots in tq40_factor_solve


def kernel_lines(text, kernel):
    """The instructions of the one kernel whose symbol contains `kernel`: from its label to its
    s_endpgm (the kernels have one exit each)."""
    labels = re.findall(r"^(\S*%s\S*):" % re.escape(kernel), text, re.M)
    assert len(labels) == 1, (kernel, labels)
    body = text[text.index("\n" + labels[0] + ":"):]
    lines = []
    for line in body.splitlines()[2:]:
        s = line.strip()
        if not line.startswith("\t") or s.startswith((".", ";")):
            continue
        lines.append(s)
        if s.startswith("s_endpgm"):
            return lines
    raise AssertionError("no s_endpgm after " + labels[0])


def count(lines, prefix):
    return len([l for l in lines if l.startswith(prefix)])


@needs_hipcc
def test_hit_kernel_runs_no_dlarfg(asm_text):  # noqa: F811
    hit = kernel_lines(asm_text, "solve_tq40_factor_kernel")
    fill = kernel_lines(asm_text, "fill_tq40_factor_kernel")
    fp64 = [l for l in hit if re.match(r"v_(mul|add|fma|fmac)_f64", l)]
    print(f"solve_tq40_factor_kernel: {len(hit)} instructions, {len(fp64)} FP64 VALU, "
          f"{count(hit, 'v_rsq_f64')} v_rsq_f64, {count(hit, 'v_rcp_f64')} v_rcp_f64, "
          f"{count(hit, 'v_cndmask_b32')} v_cndmask_b32; "
          f"fill_tq40_factor_kernel: {count(fill, 'v_rsq_f64')} v_rsq_f64")
    assert count(hit, "v_rsq_f64") == SQRTS
    assert count(fill, "v_rsq_f64") == STEPS + SQRTS
    assert len(hit) < HIT_BEFORE, len(hit)


@needs_hipcc
def test_fill_kernel_keeps_its_reduction(asm_text):  # noqa: F811
    fill = kernel_lines(asm_text, "fill_tq40_factor_kernel")
    dpp = count(fill, "v_fmac_f64_dpp")
    both = len(re.findall(r"^\tv_fmac_f64_dpp", asm_text, re.M))
    print(f"fill_tq40_factor_kernel: {len(fill)} instructions, {dpp} v_fmac_f64_dpp "
          f"({both} in the file)")
    # test_isa_factor.py's bound on the file, here on the fill kernel alone
    assert dpp > 3000, dpp
