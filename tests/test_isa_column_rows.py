"""Resource checks of the level kernels of CWBL_OPT_COLUMN_ROWS (CPU: compiles
cwbl_tq_rows_column.hip and cwbl_tq_rows_factor.hip to gfx950 assembly and reads the kernels'
metadata only, test_isa_column_factor.py's method).  solve_tqb_factor_column_kernel<128, 64> and
solve_tqb_factor_column_all_kernel<128, 64> run the half-row hit's body per level and have to fit
what that kernel fits: no scratch, at most 256 VGPRs (two waves per SIMD) and the LDS of
solve_tqb_factor_kernel<128, 64>, which is TailSmem<128, 64>.  The hit kernel, whose body became a
function for them, and the fill keep the figures DESIGN.md §3.9 states: 220 and 219 VGPRs, no
scratch.  The file of the level kernels holds these two and no other."""
import re

from test_isa import needs_hipcc
from test_isa_column_factor import metadata

ROWS = r"_ZN4cwbl%sILi128ELi64EEEv"


def one(seen, name):
    hits = [f for n, f in seen.items() if re.match(ROWS % name, n)]
    assert len(hits) == 1, (name, sorted(seen))
    return hits[0]


@needs_hipcc
def test_level_kernels_fit_the_hit_kernel(tmp_path):
    new = metadata(tmp_path, "cwbl_tq_rows_column")
    old = metadata(tmp_path, "cwbl_tq_rows_factor")
    assert len(new) == 2 and len(old) == 2, (sorted(new), sorted(old))
    hit = one(old, "23solve_tqb_factor_kernel")
    fill = one(old, "20fill_tqb_tail_kernel")
    for name in ("30solve_tqb_factor_column_kernel", "34solve_tqb_factor_column_all_kernel"):
        vgpr, lds, scratch = one(new, name)
        print(f"{name[2:]}<128, 64>: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch")
        assert scratch == 0, (name, scratch)
        assert vgpr <= 256, (name, vgpr)
        assert lds == hit[1], (name, lds, hit[1])
    print(f"solve_tqb_factor_kernel<128, 64>: {hit}; fill_tqb_tail_kernel<128, 64>: {fill}")
    assert (hit[0], hit[2]) == (220, 0), hit
    assert (fill[0], fill[2]) == (219, 0), fill
