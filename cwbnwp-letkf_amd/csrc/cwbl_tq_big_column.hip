// cwbl_tq_big_column.hip — the level kernel of a column-shared call on the hand-off path at
// KP = 96 (CWBL_OPT_COLUMN_FACTOR with CWBL_OPT_COLUMN_SHARE, k = 65..96):
//   solve_tqb_factor_column_kernel<KP, J0>  the levels 1 .. nz-1 of a column from the
//                                           BigFactor<KP, J0> that the hand-off kernel and
//                                           fill_tqb_tail_kernel<KP, J0> left when they analysed
//                                           level 0 on the column view.
// One column per wavefront; blockIdx.y selects a range of lw levels.  The neighbour lists, A,
// b1, the factor, the trace and so the quadrature level are the column's; a
// level brings its own x' only.  A level is solve_tqb_factor_kernel's body (tqb_factor_hit,
// cwbl_tq_big_factor.h) at the level's var index, so its bits are the hit kernel's, which are
// the kernel pair's.  The factor (4977 words) does not fit the registers of two waves per SIMD,
// so every level streams it again: it is the wavefront's own and has just been read (L2 /
// MALL).  Nothing in a level's text depends on the level but its x', so the compiler would move
// the loads, the lane masks and the addresses out of the level loop into registers that are not
// there; the factor's address and the lane are redefined per level (an asm the compiler cannot
// see through, as touch / touched in the tq40 kernels), which keeps them in.
//
// The kernel stores no info: it is the fill's, per column.  A column with p = 0 leaves at once.
#include "cwbl_tq_big_factor.h"

namespace cwbl {

template <int KP, int J0>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_column_kernel(SolveConsts c, SlabDev slab, long long g0, int ncol, int nz, int lw,
                               const double *__restrict__ fac, const int2 *__restrict__ info) {
  using SM = TailSmem<KP, J0>;
  __shared__ SM sm;

  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);  // the tail's XCD-chunk order
  if (gi >= ncol) return;
  const int kz0 = 1 + (int)blockIdx.y * lw, kz1 = min(nz, kz0 + lw);  // levels [kz0, kz1)
  if (kz0 >= kz1) return;
  const int l = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var stays as it is at every level

  // the column's point at level 0 (g0 + gi < ix_lim iy_lim); level kz lies nx ny kz further
  const long long P0 = bf_point_index(slab, g0 + gi);
  const long long nxy = (long long)slab.nx * slab.ny;
  for (int kz = kz0; kz < kz1; ++kz) {
    // the previous level has read sm (one wavefront: the barrier orders the LDS accesses)
    if (kz != kz0) __syncthreads();
    // redefined per level: the factor's address, and the lane, which the masks, the lane offsets
    // and the LDS addresses of a level derive from
    const double *fp = fac;
    int ll = l;
    asm volatile("" : "+s"(fp), "+v"(ll));
    tqb_factor_hit<KP, J0, false>(sm, c, slab, gi, ll, k, P0 + nxy * kz, fp, ptot, nullptr);
  }
}

hipError_t launch_solve_tqb_factor_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                          long long g0, int ncol, int nz, int lw,
                                          const double *fac, const int2 *info) {
  // KP = 128 (CWBL_OPT_COLUMN_ROWS): cwbl_tq_rows_column.hip
  if (kp == 128)
    return launch_solve_tqb_factor_column_rows(s, c, slab, g0, ncol, nz, lw, fac, info);
  if (ncol <= 0 || nz < 2) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !fac || !info || lw < 1 ||
      slab.nz != nz || g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz - 1 + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_column_kernel<96, 32>),
                     dim3((unsigned)ncol, (unsigned)ranges), dim3(64), 0, s, c, slab, g0, ncol, nz,
                     lw, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
