// cwbl_tq40_column.hip — solve_tq40_column_kernel<KP>: solve_tq40_kernel (cwbl_tq40.hip) for
// the levels of a column whose obs types all localise in 2-D (CWBL_OPT_COLUMN_SHARE = 1).
//
// With no vertical localisation the neighbour list of a grid point, and so A = inflat I +
// Yb Yb^T, b1 = Yb d and the factor A = Q T Q^T, depend on the point's column only; the level
// enters through x' and the epilogue.  A level of the column is to the solve what a variable
// of a group is to solve_tq40_multi_kernel: another x' run through the same factor.  So the
// body is that kernel's, tq40_passes (cwbl_tq40_passes.h), with a level as the pass
// (Tq40LevelPasses):
//   - blockIdx.y selects the level range [lw blockIdx.y, + lw): each wave of a range repeats
//     the tridiagonalisation (the host splits the levels only where the columns alone do not
//     fill the device), and the result does not depend on lw;
//   - info is written once per column, by the wave of the first range.  A column without
//     accepted obs (p = 0) is left untouched at every level.
// Each level's analysis equals solve_tq40_kernel's on the same record and under the same
// quadrature rule bit for bit.  The rule is the wave's (tq40_wave_rounds: the largest round
// class of its four points), and this kernel's waves hold four consecutive COLUMNS where
// solve_tq40_kernel's hold four consecutive points of the slab: the same sets when
// ix_lim iy_lim is a multiple of 4.  Otherwise a point whose two waves differ in class runs a
// longer rule in one of them, and the low bits of its analysis may differ between the two
// kernels (include/cwb_letkf_core.h, cwbl_column_info).
#include "cwbl_tq40_passes.h"

namespace cwbl {

template <int KP>
__global__ void __launch_bounds__(64, 2)
solve_tq40_column_kernel(SolveConsts c, SlabDev slab, long long g0, int npts, int nz, int lw,
                         double *__restrict__ ws, int2 *__restrict__ info) {
  tq40_passes<KP>(c, slab, Tq40LevelPasses{c, slab, nz, lw}, g0, npts, ws, info);
}

hipError_t launch_solve_tq40_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                    long long g0, int npts, int nz, int lw, double *ws,
                                    int2 *info) {
  if (npts <= 0 || nz <= 0) return hipSuccess;
  if (c.quad_r == nullptr || kp != kTq4KP || lw < 1) return hipErrorInvalidValue;
  const dim3 grid((npts + 3) / 4, (nz + lw - 1) / lw);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tq40_column_kernel<kTq4KP>), grid, dim3(64), 0, s, c, slab, g0, npts,
                     nz, lw, ws, info);
  return hipGetLastError();
}

}  // namespace cwbl
