// cwbl_tq_rows_column.hip — the level kernels of a column-shared call on the hand-off path at
// KP = 128 (k = 97..128; CWBL_OPT_COLUMN_ROWS with CWBL_OPT_COLUMN_FACTOR or
// CWBL_OPT_COLUMN_REUSE):
//   solve_tqb_factor_column_kernel<128, 64>      the levels 1 .. nz-1 of a column from the
//                                                BigFactor<128, 64> that the half-row hand-off
//                                                kernel and fill_tqb_tail_kernel<128, 64> left
//                                                when they analysed level 0 on the column view;
//   solve_tqb_factor_column_all_kernel<128, 64>  the same started at level 0: every level of a
//                                                column whose factor the column cache kept, and a
//                                                call of one level (MU).
// They specialise the KP = 96 templates of cwbl_tq_big_column.hip and cwbl_tq_big_column_all.hip,
// whose launchers pass KP = 128 on to the two at the end of this file.  One column per wavefront;
// blockIdx.y selects a range of lw levels.  The neighbour lists, A, b1, the factor, the trace and
// so the quadrature level are the column's; a level brings its own x' only.  A
// level is the half-row hit's body (tqb_rows_hit, cwbl_tq_rows_factor.h: the body of
// solve_tqb_factor_kernel<128, 64>) at the level's var index, so its bits are the hit kernel's,
// which are the kernel pair's.  The factor (8705 words) does not fit the registers, so every
// level streams it again through the ring: it is the wavefront's own and has just been read
// (L2 / MALL).  Nothing in a level's text depends on the level but its x', so the compiler would
// move the loads, the lane masks and the addresses out of the level loop into registers that are
// not there; the factor's address and the lane are redefined per level (an asm the compiler
// cannot see through, as in cwbl_tq_big_column.hip), which keeps them in.
//
// The kernels store no info: it is the fill's, per column.  A column with p = 0 leaves at once.
// Two waves per SIMD, the hit kernel's bound: three were never available for this body
// (DESIGN.md §3.9).
#include "cwbl_tq_rows_factor.h"

namespace cwbl {

namespace {

// The levels kzf + lw blockIdx.y .. of column blockIdx.x (through xcd_remap_rev) from the
// BigFactor<128, 64> at fac + gi WORDS.  sm is the workgroup's own; info is read only.
__device__ __forceinline__ void tqb_rows_levels(TailSmem<128, 64> &sm, const SolveConsts &c,
                                                const SlabDev &slab, long long g0, int ncol,
                                                int nz, int lw, int kzf,
                                                const double *__restrict__ fac,
                                                const int2 *__restrict__ info) {
  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);  // the tail's XCD-chunk order
  if (gi >= ncol) return;
  const int kz0 = kzf + (int)blockIdx.y * lw, kz1 = min(nz, kz0 + lw);  // levels [kz0, kz1)
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
    tqb_rows_hit<false>(sm, c, slab, gi, ll, k, P0 + nxy * kz, fp, ptot, nullptr);
  }
}

}  // namespace

template <int KP, int J0>
__global__ void solve_tqb_factor_column_kernel(SolveConsts c, SlabDev slab, long long g0, int ncol,
                                               int nz, int lw, const double *__restrict__ fac,
                                               const int2 *__restrict__ info);
template <int KP, int J0>
__global__ void solve_tqb_factor_column_all_kernel(SolveConsts c, SlabDev slab, long long g0,
                                                   int ncol, int nz, int lw,
                                                   const double *__restrict__ fac,
                                                   const int2 *__restrict__ info);

template <>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_column_kernel<128, 64>(SolveConsts c, SlabDev slab, long long g0, int ncol,
                                        int nz, int lw, const double *__restrict__ fac,
                                        const int2 *__restrict__ info) {
  __shared__ TailSmem<128, 64> sm;
  tqb_rows_levels(sm, c, slab, g0, ncol, nz, lw, 1, fac, info);
}

template <>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_column_all_kernel<128, 64>(SolveConsts c, SlabDev slab, long long g0, int ncol,
                                            int nz, int lw, const double *__restrict__ fac,
                                            const int2 *__restrict__ info) {
  __shared__ TailSmem<128, 64> sm;
  tqb_rows_levels(sm, c, slab, g0, ncol, nz, lw, 0, fac, info);
}

hipError_t launch_solve_tqb_factor_column_rows(hipStream_t s, SolveConsts c, SlabDev slab,
                                               long long g0, int ncol, int nz, int lw,
                                               const double *fac, const int2 *info) {
  if (ncol <= 0 || nz < 2) return hipSuccess;
  if (c.quad == nullptr || c.k <= 128 - 62 || c.k > 128 || !fac || !info || lw < 1 ||
      slab.nz != nz || g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz - 1 + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_column_kernel<128, 64>),
                     dim3((unsigned)ncol, (unsigned)ranges), dim3(64), 0, s, c, slab, g0, ncol, nz,
                     lw, fac, info);
  return hipGetLastError();
}

hipError_t launch_solve_tqb_factor_column_all_rows(hipStream_t s, SolveConsts c, SlabDev slab,
                                                   long long g0, int ncol, int nz, int lw,
                                                   const double *fac, const int2 *info) {
  if (ncol <= 0 || nz < 1) return hipSuccess;
  if (c.quad == nullptr || c.k <= 128 - 62 || c.k > 128 || !fac || !info || lw < 1 ||
      slab.nz != nz || g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_column_all_kernel<128, 64>),
                     dim3((unsigned)ncol, (unsigned)ranges), dim3(64), 0, s, c, slab, g0, ncol, nz,
                     lw, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
