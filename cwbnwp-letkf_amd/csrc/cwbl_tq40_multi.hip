// cwbl_tq40_multi.hip — solve_tq40_multi_kernel<KP>: solve_tq40_kernel (cwbl_tq40.hip) for a
// group of variables that share a localisation (cwbl_analyze_vars).
//
// The body is tq40_passes (cwbl_tq40_passes.h: one tridiagonalisation per point, then one
// replay, quadrature, back-transform and epilogue per pass) with a variable of the group as
// the pass: var, flags and alphas from the by-value tables of Tq40Vars, and every wave writes
// its points' info.
#include "cwbl_tq40_passes.h"

namespace cwbl {

template <int KP>
__global__ void __launch_bounds__(64, 2)
solve_tq40_multi_kernel(SolveConsts c, SlabDev slab, Tq40Vars vars, long long g0, int npts,
                        double *__restrict__ ws, int2 *__restrict__ info) {
  tq40_passes<KP>(c, slab, Tq40GroupPasses{vars}, g0, npts, ws, info);
}

hipError_t launch_solve_tq40_multi(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   const Tq40Vars &vars, long long g0, int npts, double *ws,
                                   int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad_r == nullptr || kp != kTq4KP || vars.nvar < 1 || vars.nvar > kMaxGroupVars)
    return hipErrorInvalidValue;
  const dim3 grid((npts + 3) / 4);
  hipLaunchKernelGGL((solve_tq40_multi_kernel<kTq4KP>), grid, dim3(64), 0, s, c, slab, vars, g0,
                     npts, ws, info);
  return hipGetLastError();
}

}  // namespace cwbl
