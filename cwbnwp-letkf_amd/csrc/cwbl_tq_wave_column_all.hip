// cwbl_tq_wave_column_all.hip — the all-levels kernel of a column-shared call that hits the
// column cache on the one-wavefront path at KP = 48, 56, 64 (CWBL_OPT_COLUMN_REUSE, k = 41..64):
//   solve_tq_wave_factor_column_all_kernel<KP>  the levels 0 .. nz-1 of a column from the
//                                               WaveFactor<KP> that an earlier call's
//                                               fill_tq_wave_kernel<KP> left in the column cache.
// It is solve_tq_wave_factor_column_kernel (cwbl_tq_wave_column.hip) started at level 0: the body
// is tq_wave_factor_levels (cwbl_tq_wave.h), that kernel's text with the first level as an
// argument, here 0 since a hit has no fill that analysed level 0 (why that kernel does not call
// the function as well: see there).  One column per wavefront; blockIdx.y selects a range
// of lw levels, and the first level of a range stores the reflectors v = x scal to LDS.  A
// level's bits are the hit kernel's, which are the single kernel's and the fill's, so the slab
// equals the filling call's for every level split.
//
// The kernel reads info (the column's accepted count, restored from the cache) and stores none.
// A column with p = 0 leaves at once.
#include "cwbl_tq_wave.h"

namespace cwbl {

template <int KP>
__global__ void __launch_bounds__(64, TqOccupancy<KP>::kWaves)
solve_tq_wave_factor_column_all_kernel(SolveConsts c, SlabDev slab, long long g0, int ncol,
                                       int nz, int lw, const double *__restrict__ fac,
                                       const int2 *__restrict__ info) {
  __shared__ TqSmem<KP> sm;
  tq_wave_factor_levels<KP>(sm, c, slab, g0, ncol, nz, lw, 0, fac, info);
}

hipError_t launch_solve_tq_wave_factor_column_all(hipStream_t s, int kp, SolveConsts c,
                                                  SlabDev slab, long long g0, int ncol, int nz,
                                                  int lw, const double *fac, const int2 *info) {
  if (ncol <= 0 || nz < 1) return hipSuccess;
  if (c.quad == nullptr || !fac || !info || lw < 1 || slab.nz != nz ||
      g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)ncol, (unsigned)ranges);
#define CWBL_TQWA_CASE(K)                                                                      \
  case K:                                                                                      \
    hipLaunchKernelGGL((solve_tq_wave_factor_column_all_kernel<K>), grid, dim3(64), 0, s, c,   \
                       slab, g0, ncol, nz, lw, fac, info);                                     \
    return hipGetLastError();
  switch (kp) {
    CWBL_TQWA_CASE(48)
    CWBL_TQWA_CASE(56)
    CWBL_TQWA_CASE(64)
    default:
      return hipErrorInvalidValue;
  }
#undef CWBL_TQWA_CASE
}

}  // namespace cwbl
