// cwbl_tq_rows_factor.hip — the factor cache's kernel pair of the hand-off path at KP = 128
// (k = 97..128, CWBL_OPT_ROWS_REUSE), behind the half-row hand-off kernel solve_tq_rows_kernel
// <128, 64> (cwbl_tq_rows.hip), which runs unchanged:
//   fill_tqb_tail_kernel<128, 64>     cwbl_tq_big_factor.h's text at this KP: solve_tqb_tail_kernel
//                                     <128, 64, 3>'s analysis (the same expressions, so the same
//                                     bits) and the point's BigFactor<128, 64>;
//   solve_tqb_factor_kernel<128, 64>  the same analysis from that factor, one point per wavefront.
//                                     Steps j < 64 replay the x' half of solve_tq_rows_kernel's
//                                     step, steps j >= 64 the tail's; tqb_finish ends it.
// The KP = 96 pair is cwbl_tq_big_factor.hip's, whose two launchers pass KP = 128 on to the two
// at the end of this file.  The hit kernel differs from that file's in two places.  The
// half-row kernel sums v . x' over four waves of which two hold x' (waves 0 and 2, rows l and
// 64 + l), so the sum is (p0 + 0) + (p1 + 0) and not (p0 + p1) + (0 + 0).  And its 64 reflectors,
// two registers each, do not fit a register file beside the tail's columns: every column is read
// by one replayed step, so the columns pass through a ring of registers in the order of their
// use.  The hit kernel's body is a function of cwbl_tq_rows_factor.h.
#include "cwbl_tq_rows_factor.h"

namespace cwbl {

namespace {
// Waves per SIMD of the hit kernel.
constexpr int kRowsHitWaves = 2;
}  // namespace

// One point per wavefront from its BigFactor<128, 64>.  info[gi].x is the accepted count the
// fill left (restored by the host); the flags and alphas are this call's.  The body is
// tqb_rows_hit (cwbl_tq_rows_factor.h), which the level kernels of a column-shared call
// (cwbl_tq_rows_column.hip, CWBL_OPT_COLUMN_ROWS) run once per level; as its caller this kernel's
// assembly equals that of the body written out here in every line (profiles/column_rows.txt).
template <>
__global__ void __launch_bounds__(64, kRowsHitWaves)
solve_tqb_factor_kernel<128, 64>(SolveConsts c, SlabDev slab, long long g0, int npts,
                                 const double *__restrict__ fac, int2 *__restrict__ info) {
  __shared__ TailSmem<128, 64> sm;

  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);  // the tail's XCD-chunk order
  if (gi >= npts) return;
  const int l = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var and info stay as they are

  const long long P = bf_point_index(slab, g0 + gi);
  tqb_rows_hit<true>(sm, c, slab, gi, l, k, P, fac, ptot, info);
}

hipError_t launch_fill_tqb_tail_rows(hipStream_t s, SolveConsts c, SlabDev slab, long long g0,
                                     int npts, double *ws, int2 *info, double *fac) {
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || c.k <= 128 - 62 || c.k > 128 || !ws || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((fill_tqb_tail_kernel<128, 64>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, ws, info, fac);
  return hipGetLastError();
}

hipError_t launch_solve_tqb_factor_rows(hipStream_t s, SolveConsts c, SlabDev slab, long long g0,
                                        int npts, const double *fac, int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || c.k <= 128 - 62 || c.k > 128 || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_kernel<128, 64>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
