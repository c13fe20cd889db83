// cwbl_tq_big_column_all.hip — the all-levels kernel of a column-shared call that hits the
// column cache on the hand-off path at KP = 96 (CWBL_OPT_COLUMN_REUSE, k = 65..96):
//   solve_tqb_factor_column_all_kernel<KP, J0>  the levels 0 .. nz-1 of a column from the
//                                               BigFactor<KP, J0> that an earlier call's hand-off
//                                               kernel and fill_tqb_tail_kernel<KP, J0> left in
//                                               the column cache.
// It is solve_tqb_factor_column_kernel (cwbl_tq_big_column.hip) started at level 0: the body is
// tqb_factor_levels (cwbl_tq_big_factor.h), that kernel's text with the first level as an
// argument, here 0 since a hit has no fill that analysed level 0 (why that kernel does not call
// the function as well: see there).  One column per wavefront; blockIdx.y selects a range of
// lw levels.  A level is solve_tqb_factor_kernel's body at the level's var index, so its bits are
// the hit kernel's, which are the kernel pair's and the fill's.
//
// The kernel reads info (the column's accepted count, restored from the cache) and stores none.
// A column with p = 0 leaves at once.
#include "cwbl_tq_big_factor.h"

namespace cwbl {

template <int KP, int J0>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_column_all_kernel(SolveConsts c, SlabDev slab, long long g0, int ncol, int nz,
                                   int lw, const double *__restrict__ fac,
                                   const int2 *__restrict__ info) {
  __shared__ TailSmem<KP, J0> sm;
  tqb_factor_levels<KP, J0>(sm, c, slab, g0, ncol, nz, lw, 0, fac, info);
}

hipError_t launch_solve_tqb_factor_column_all(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                              long long g0, int ncol, int nz, int lw,
                                              const double *fac, const int2 *info) {
  // KP = 128 (CWBL_OPT_COLUMN_ROWS): cwbl_tq_rows_column.hip
  if (kp == 128)
    return launch_solve_tqb_factor_column_all_rows(s, c, slab, g0, ncol, nz, lw, fac, info);
  if (ncol <= 0 || nz < 1) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !fac || !info || lw < 1 ||
      slab.nz != nz || g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_column_all_kernel<96, 32>),
                     dim3((unsigned)ncol, (unsigned)ranges), dim3(64), 0, s, c, slab, g0, ncol, nz,
                     lw, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
