// cwbl_tq_big_factor.hip — the factor cache's kernel pair of the hand-off path at KP = 96
// (k = 65..96, CWBL_OPT_BIG_REUSE):
//   fill_tqb_tail_kernel<KP, J0>     solve_tqb_tail_kernel<KP, J0, 2>'s analysis (cwbl_tq_tail.hip:
//                                    the same text, so the same bits) from the hand-off kernel's
//                                    record, which also leaves the point's factor as a
//                                    BigFactor<KP, J0> (cwbl_internal.h) with plain vector stores
//                                    that nothing waits for: its own pivot rows as each step forms
//                                    them, the hand-off kernel's reflectors as the back-transform
//                                    loads them, T, Q^T b1, tau and scal after the loop;
//   solve_tqb_factor_kernel<KP, J0>  the same analysis from that factor, one point per wavefront:
//                                    no lists, no assembly, no hand-off kernel, no record and no
//                                    dlarfg.  It replays the x' half of every step — steps j < J0
//                                    in the hand-off kernel's expressions and layout, steps
//                                    j >= J0 in the tail's — and then runs the quadrature, the
//                                    back-transform and the epilogue both kernels share
//                                    (tqb_finish).
// Shared with solve_tqb_tail_kernel through cwbl_tq_tail_common.h: the shared-memory struct
// (TailSmem), the point index and the fp32 readlane.  Both kept every kernel's instruction
// stream as it was (profiles/twin_merge.txt).  The two larger texts are still repeated, in
// cwbl_tq_big_factor.h (which the KP = 128 pair, cwbl_tq_rows_factor.hip, shares),
// because solve_tqb_tail_kernel, with either as a shared function, compiled to other vector
// code than with its own text (the numbers are in cwbl_tq_tail_common.h): the fill's hand-off
// load and Householder loop are the tail's with the factor's stores added, and tqb_finish is
// the tail's quadrature, back-transform and epilogue as a function over two row loaders.
#include "cwbl_tq_big_factor.h"

namespace cwbl {

// One point per wavefront from its BigFactor.  info[gi].x is the accepted count the fill left
// (restored by the host); the flags and alphas are this call's.  The body is tqb_factor_hit
// (cwbl_tq_big_factor.h), which the level kernel of a column-shared call runs per level
// (cwbl_tq_big_column.hip).
//
// Steps j < J0 are replayed as the hand-off kernel's waves 0 and 1 hold x': one register with
// row = lane, one with rows 64 .. KP-1 on lanes < KP - 64 and zeros elsewhere; v . x' is summed
// as its bsum4 sums it (a wave sum per wave, then (w0 + w1) + (w2 + w3), the two waves past KP
// adding zeros).  Steps j >= J0 run in the tail's layout (lane l is row J0 + l) and expressions.
// The loads are unconditional, each a constant offset from one lane offset into the point's own
// factor (a load under a lane mask is a branch of its own, and the waits behind such branches
// come out as vmcnt(0)); the row mask is applied at the use.  They are issued in the order of
// first use: the scalars and the J0 reflectors (two registers each) before step 0, two of the
// tail's columns behind each replayed step into the registers it released (all KP (KP - 1) / 2
// words at once do not fit the register file at two waves per SIMD), T and Q^T b1 last.
template <int KP, int J0>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                        const double *__restrict__ fac, int2 *__restrict__ info) {
  using SM = TailSmem<KP, J0>;
  __shared__ SM sm;

  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);  // the tail's XCD-chunk order
  if (gi >= npts) return;
  const int l = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var and info stay as they are

  const long long P = bf_point_index(slab, g0 + gi);
  tqb_factor_hit<KP, J0>(sm, c, slab, gi, l, k, P, fac, ptot, info);
}

hipError_t launch_fill_tqb_tail(hipStream_t s, int kp, SolveConsts c, SlabDev slab, long long g0,
                                int npts, double *ws, int2 *info, double *fac) {
  if (kp == 128) return launch_fill_tqb_tail_rows(s, c, slab, g0, npts, ws, info, fac);
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !ws || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((fill_tqb_tail_kernel<96, 32>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, ws, info, fac);
  return hipGetLastError();
}

hipError_t launch_solve_tqb_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   long long g0, int npts, const double *fac, int2 *info) {
  if (kp == 128) return launch_solve_tqb_factor_rows(s, c, slab, g0, npts, fac, info);
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_kernel<96, 32>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
