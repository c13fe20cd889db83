"""Resource checks of the all-levels kernels of CWBL_OPT_COLUMN_REUSE (CPU: compiles
cwbl_tq_wave_column_all.hip and cwbl_tq_big_column_all.hip to gfx950 assembly and reads the
kernels' metadata only, test_isa_column_factor.py's method): each is the level kernel of
CWBL_OPT_COLUMN_FACTOR started at level 0 and has to fit what that kernel fits.
solve_tq_wave_factor_column_all_kernel<KP> at KP = 48, 56, 64 is free of scratch, keeps the waves
per SIMD of TqOccupancy<KP> (at most 512 // waves(KP) VGPRs) and uses no more LDS than
solve_tq_kernel<KP>'s TqSmem<KP>; solve_tqb_factor_column_all_kernel<96, 32> is free of scratch,
stays within 256 VGPRs and uses no more LDS than the tail's TailSmem<96, 32>.  Each file holds
these kernels and no other."""
import re

from test_isa import needs_hipcc
from test_isa_column_factor import TAIL_LDS, metadata
from test_isa_tq_multi import LDS, waves


@needs_hipcc
def test_wave_column_all_budgets(tmp_path):
    seen = {}
    for name, figures in metadata(tmp_path, "cwbl_tq_wave_column_all").items():
        m = re.match(r"_ZN4cwbl38solve_tq_wave_factor_column_all_kernelILi(\d+)EEEv", name)
        assert m, name
        seen[int(m.group(1))] = figures
    assert sorted(seen) == [48, 56, 64], sorted(seen)
    for kp, (vgpr, lds, scratch) in sorted(seen.items()):
        print(f"solve_tq_wave_factor_column_all_kernel<{kp}>: {vgpr} VGPRs, {lds} B LDS, "
              f"{scratch} B scratch")
        assert scratch == 0, (kp, scratch)
        assert vgpr <= 512 // waves(kp), (kp, vgpr)
        assert lds <= LDS[kp], (kp, lds)


@needs_hipcc
def test_big_column_all_budgets(tmp_path):
    seen = metadata(tmp_path, "cwbl_tq_big_column_all")
    assert len(seen) == 1, sorted(seen)
    (name, (vgpr, lds, scratch)), = seen.items()
    assert re.match(r"_ZN4cwbl34solve_tqb_factor_column_all_kernelILi96ELi32EEEv", name), name
    print(f"solve_tqb_factor_column_all_kernel<96, 32>: {vgpr} VGPRs, {lds} B LDS, "
          f"{scratch} B scratch")
    assert scratch == 0, scratch
    assert vgpr <= 256, vgpr
    assert lds <= TAIL_LDS, lds
