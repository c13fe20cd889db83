// cwbl_tq_wave_column.hip — the level kernel of a column-shared call on the one-wavefront path
// at KP = 48, 56, 64 (CWBL_OPT_COLUMN_FACTOR with CWBL_OPT_COLUMN_SHARE, k = 41..64):
//   solve_tq_wave_factor_column_kernel<KP>  the levels 1 .. nz-1 of a column from the
//                                           WaveFactor<KP> that fill_tq_wave_kernel<KP> left when
//                                           it analysed level 0 on the column view.
// One column per wavefront; blockIdx.y selects a range of lw levels.  The neighbour lists, A,
// b1, the factor, the trace and so the quadrature level are the column's; a
// level brings its own x' only.  Per level the kernel runs solve_tq_wave_factor_kernel's replay
// (cwbl_tq_wave.hip: the same expressions in the same order, the fill's slot of wave_sum4_dpp)
// and tq_wave_finish, so a level's bits are the hit kernel's, which are the single kernel's.
// What does not depend on the level is done once per wavefront: the loads of T and Q^T b1,
// their stores and tau's to sm.tq and sm.tau, the trace and the quadrature level it selects, and
// the reflectors v = x scal in LDS
// (the first level of the range stores them, the others read them in the back-transform).
//
// The columns x (and the steps' scal and tau beside them) are loaded again per level, in the hit
// kernel's order: they are the wavefront's own and have just been read (L2).  Held in registers
// across the levels they do not fit TqOccupancy<KP> at any KP: the columns (2 (KP - 2) VGPRs)
// would be live together with tq_wave_finish's recurrence arrays (2 KP VGPRs), and the compiler
// reports 284, 52 and 188 B of scratch at KP = 48, 56 and 64.
//
// Nothing in a level's text depends on the level but its x', so the compiler would move the
// loads, the lane masks and the LDS addresses out of the level loop and keep them in registers
// it does not have (132, 308 and 28 B of scratch).  The asm redefinitions below (the lane and
// the factor's lane base, once per level) stop that, as touch / touched do in the tq40 kernels
// (§3.1).
//
// The kernel stores no info: it is the fill's, per column.  A column with p = 0 leaves at once.
#include "cwbl_tq_wave.h"

namespace cwbl {

template <int KP>
__global__ void __launch_bounds__(64, TqOccupancy<KP>::kWaves)
solve_tq_wave_factor_column_kernel(SolveConsts c, SlabDev slab, long long g0, int ncol, int nz,
                                   int lw, const double *__restrict__ fac,
                                   const int2 *__restrict__ info) {
  static_assert(KP % 8 == 0 && KP > 40 && KP <= 64, "KP");
  using SM = TqSmem<KP>;
  using F = WaveFactor<KP>;
  constexpr int NS = KP - 2;  // steps with a reflector at k = KP
  __shared__ SM sm;

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= ncol) return;
  const int kz0 = 1 + (int)blockIdx.y * lw, kz1 = min(nz, kz0 + lw);  // levels [kz0, kz1)
  if (kz0 >= kz1) return;
  const int lane0 = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var stays as it is at every level

  // the column's point at level 0 (g0 + gi < ix_lim iy_lim); level kz lies nx ny kz further
  const long long P0 = wave_point_index(slab, g0 + gi);
  const long long nxy = (long long)slab.nx * slab.ny;
  double trace = 0.0;
  // the hit kernel's lane base: unconditional loads at constant offsets, masks at the use
  const auto *f0 = gptr(fac + (long long)gi * F::WORDS) + (lane0 < KP ? lane0 : KP - 1);
  {
    const double tauv = f0[F::TAU], dv = f0[F::D], cv = f0[F::C], u1 = f0[F::U1];
    // sm.tq's level-independent columns and sm.tau as the single kernel's loop leaves them
    if (lane0 < KP) {
      sm.tq[lane0][0] = dv;
      sm.tq[lane0][1] = cv;
      sm.tq[lane0][2] = u1;
      sm.tau[lane0] = tauv;
    }
    if (lane0 == 0) sm.tq[KP][1] = 0.0;
    // trace A = sum of T's live diagonal, added in the steps' order
    for (int j = 0; j < k; ++j) trace += readlane_f64(dv, j);
  }
  // the quadrature level, from the spectrum bound M / m = trace / inflat - (k - 1): the column's
  const double ratio = trace / (double)c.inflat - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }

  for (int kz = kz0; kz < kz1; ++kz) {
    // the lane, redefined per level: the masks and the LDS addresses of a level derive from it
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const long long P = P0 + nxy * kz;
    float xbl = 0.0f;
    if (lane < k) xbl = slab.var[P + slab.L * lane];
    __builtin_amdgcn_sched_barrier(0);
    // the steps' scalars and the columns, in the order of first use
    // (solve_tq_wave_factor_kernel); the base is redefined per level, so the loads stay in the
    // loop
    auto *f = f0;
    asm volatile("" : "+v"(f));
    const double tauw = f[F::TAU], scalw = f[F::SCAL];
    __builtin_amdgcn_sched_barrier(0);
    double x[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      static_assert(F::COL >= NS, "a lane above row j + 1 stays inside the factor");
      x[j] = f[F::col(j) - (j + 1)];
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("" : "+v"(xbl));  // the wait for xbl alone, ahead of the loop that sums it
    const double xb_mean = wave_xb_mean(xbl, k, c.nmember_inv);
    double ux = (lane < k) ? (double)xbl - xb_mean : 0.0;  // x', becomes Q^T x'
    // the previous level's back-transform has read sm.u.reg and sm.tq (one wavefront: the
    // barrier orders the LDS accesses)
    __syncthreads();
    const bool first = kz == kz0;  // (uniform) this level stores the reflectors
    // ---- the x' half of every step (solve_tq_kernel's step: the same expressions) ---------
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const double tau = readlane_f64(tauw, j), scal = readlane_f64(scalw, j);
      // not the trailing 2x2 block, and not H_j = I (both uniform)
      if (j < k - 2 && !(tau == 0.0)) {
        // the fill's slot of wave_sum4_dpp (the sum's bits do not depend on it; a NaN's might)
        const double xj = (lane > j + 1 && lane < k) ? x[j] : 0.0;  // the fill's masked x
        double p0 = 0.0, xux = xj * ux, p2 = 0.0, p3 = 0.0;
        wave_sum4_dpp(p0, xux, p2, p3);
        const double v = lane == j + 1 ? 1.0 : xj * scal;
        if (first && lane > j && lane < k)
          sm.u.reg[j * (k - 1) - j * (j - 1) / 2 + lane - (j + 1)] = v;
        const double s2 = fma(scal, xux, readlane_f64(ux, j + 1));  // v . ux
        ux = fma(-tau * s2, v, ux);
      }
    }
    if (lane < KP) sm.tq[lane][3] = ux;
    __syncthreads();
    tq_wave_finish<KP>(sm, c, slab, gi, lane, k, P, xbl, xb_mean, ratio, level, dec, ptot,
                       nullptr);
  }
}

hipError_t launch_solve_tq_wave_factor_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                              long long g0, int ncol, int nz, int lw,
                                              const double *fac, const int2 *info) {
  if (ncol <= 0 || nz < 2) return hipSuccess;
  if (c.quad == nullptr || !fac || !info || lw < 1 || slab.nz != nz ||
      g0 + ncol > (long long)slab.ix_lim * slab.iy_lim)
    return hipErrorInvalidValue;
  const long long ranges = ((long long)nz - 1 + lw - 1) / lw;
  if (ranges > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)ncol, (unsigned)ranges);
#define CWBL_TQWC_CASE(K)                                                                     \
  case K:                                                                                     \
    hipLaunchKernelGGL((solve_tq_wave_factor_column_kernel<K>), grid, dim3(64), 0, s, c, slab, \
                       g0, ncol, nz, lw, fac, info);                                          \
    return hipGetLastError();
  switch (kp) {
    CWBL_TQWC_CASE(48)
    CWBL_TQWC_CASE(56)
    CWBL_TQWC_CASE(64)
    default:
      return hipErrorInvalidValue;
  }
#undef CWBL_TQWC_CASE
}

}  // namespace cwbl
