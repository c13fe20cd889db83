// cwbl_tq_wave.hip — the factor cache's kernel pair of the one-wavefront path at KP = 48, 56, 64
// (CWBL_OPT_WAVE_REUSE):
//   fill_tq_wave_kernel<KP>          solve_tq_kernel<KP, false>'s analysis (cwbl_tq.hip: the same
//                                    text, so the same bits), which also leaves the point's
//                                    factor A = Q T Q^T, the steps' scalars and Q^T b1 as a
//                                    WaveFactor<KP> (cwbl_internal.h);
//   solve_tq_wave_factor_kernel<KP>  the same analysis from that factor: no lists, no assembly,
//                                    no tridiagonalisation and no dlarfg.  It replays the x' half
//                                    of every step, the same expressions in the same order, and
//                                    then runs the quadrature, the back-transform and the epilogue
//                                    that both kernels share (tq_wave_finish).
// A hit streams WORDS x 8 B per point (18.7 KB at KP = 64) behind a serial chain of k - 2 steps
// (a product, one wave sum, two FMAs each).  Every load of the factor is issued before the first
// step, in the order of first use, one column per register, unconditionally (the lane mask is
// applied at the use), so that each step's s_waitcnt counts the loads behind its own: the chain
// then waits for the memory's latency once, at step 0, and for bandwidth after that.
#include "cwbl_tq_wave.h"

namespace cwbl {

// fac: the WaveFactor<KP> of point gi of the launch at fac + gi WORDS.  A point with p = 0
// writes none (a hit leaves at its info); a step that leaves early (j >= k - 2) or is the
// identity (tau = 0) writes no column, and a hit reads none there.
template <int KP>
__global__ void __launch_bounds__(64, TqOccupancy<KP>::kWaves)
fill_tq_wave_kernel(const TreeDesc *__restrict__ trees, SolveConsts c, SlabDev slab, long long g0,
                    int npts, const int *__restrict__ nbr_cnt, const int *__restrict__ nbr_idx,
                    int2 *__restrict__ info, double *__restrict__ fac) {
  static_assert(kTqMfmaAssembly, "the copy of solve_tq_kernel's matrix-core assembly");
  static_assert(KP % 8 == 0 && KP > 40 && KP <= 64 && TqSmem<KP>::J0T == KP,
                "the 4x4 phase only");
  constexpr int H = KP / 2;
  constexpr int NBL = AsmLayout<KP>::NBL, NBLK = AsmLayout<KP>::NBLK;
  using SM = TqSmem<KP>;
  using F = WaveFactor<KP>;
  __shared__ SM sm;

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= npts) return;
  const int lane = threadIdx.x;
  const int k = c.k;

  float3 pt = make_float3(0.0f, 0.0f, 0.0f);  // the point's projected x, y and altitude
  float xbl = 0.0f;                            // background of member `lane`
  const long long g = g0 + gi;
  const long long P = wave_point_index(slab, g);  // var index of member 0
  if (lane < k) xbl = slab.var[P + slab.L * lane];
  slab_point(slab, g, pt.x, pt.y, pt.z);
  double *__restrict__ const f = fac + (long long)gi * F::WORDS;

  int bi[NBL], bj[NBL];
  block_of_lane<KP>(lane, bi, bj);
  double acc[NBL][16];
  double b1acc;
  int ptot;
  {
    f64x4 tile[MfmaLayout<KP>::NTL];
    assemble_point_mfma<KP, kTqChunk, false>(sm.u.ch, trees, c, gi, lane, nbr_cnt, nbr_idx, pt,
                                             nullptr, nullptr, nullptr, tile, b1acc, ptot);
    if (ptot == 0) {
      if (lane == 0 && info) info[gi] = make_int2(0, 0);
      return;
    }
    // MFMA tiles -> LDS (two row halves) -> 4x4 register blocks
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int t = 0;
#pragma unroll
      for (int I = 0; I < MfmaLayout<KP>::NT; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J, ++t) {
          const int col = 16 * J + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + (lane >> 4) + 4 * r;
            if (row / H == half && row < KP && col < KP) sm.u.ah[row - half * H][col] = tile[t][r];
            if (MfmaLayout<KP>::YO_ROW && half == 0 && row == KP && col < KP)
              sm.wb[col] = tile[t][r];  // row KP of Y' Y'^T = Yb d
          }
        }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < NBL; ++it) {
        if (lane + 64 * it < NBLK && (4 * bi[it]) / H == half) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double *src = &sm.u.ah[4 * bi[it] + r - half * H][4 * bj[it]];
            const double2 x0 = *reinterpret_cast<const double2 *>(src);
            const double2 x1 = *reinterpret_cast<const double2 *>(src + 2);
            acc[it][4 * r] = x0.x; acc[it][4 * r + 1] = x0.y;
            acc[it][4 * r + 2] = x1.x; acc[it][4 * r + 3] = x1.y;
          }
        }
      }
      __syncthreads();
    }
    if (MfmaLayout<KP>::YO_ROW && lane < KP) b1acc = sm.wb[lane];
  }
  const double inflat_r8 = (double)c.inflat;
#pragma unroll
  for (int it = 0; it < NBL; ++it) {
    if (lane + 64 * it < NBLK && bi[it] == bj[it]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 4 * bi[it] + r;
        acc[it][5 * r] = ii < k ? acc[it][5 * r] + inflat_r8 : 1.0;
      }
    }
  }
  if (lane < KP) {  // padding of T: decoupled unit rows
    sm.tq[lane][0] = 1.0;
    sm.tq[lane][1] = 0.0;
    sm.tau[lane] = 0.0;
  }
  if (lane == 0) sm.tq[KP][1] = 0.0;
  __syncthreads();
  const double xb_mean = wave_xb_mean(xbl, k, c.nmember_inv);
  double ux = (lane < k) ? (double)xbl - xb_mean : 0.0;  // x', becomes Q^T x'
  double ub = (lane < KP) ? b1acc : 0.0;                  // Yb d, becomes Q^T b1

  // ---- Householder tridiagonalisation (lower, dsytd2 order): solve_tq_kernel's 4x4 phase ---
  double trace = 0.0;
  auto ld4 = [](const double *p, double (&o)[4]) {
    const double2 a0 = *reinterpret_cast<const double2 *>(p);
    const double2 a1 = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = a0.x; o[1] = a0.y; o[2] = a1.x; o[3] = a1.y;
  };
  auto step = [&](const int j, auto q, double (&A)[NBL][16]) __attribute__((always_inline)) {
    constexpr int qj = decltype(q)::value;  // column within the block: constant
    const int J = j >> 2;
#pragma unroll
    for (int it = 0; it < NBL; ++it) {
      if (lane + 64 * it < NBLK && bj[it] == J) {  // publish column j
        *reinterpret_cast<double2 *>(&sm.col[4 * bi[it]]) =
            make_double2(A[it][qj], A[it][4 + qj]);
        *reinterpret_cast<double2 *>(&sm.col[4 * bi[it] + 2]) =
            make_double2(A[it][8 + qj], A[it][12 + qj]);
      }
    }
    __syncthreads();
    const double dj = sm.col[j];
    trace += dj;
    if (lane == 0) sm.tq[j][0] = dj;
    if (j >= k - 2) {  // trailing 2x2 block: already tridiagonal
      if (j == k - 2 && lane == 0) {
        sm.tq[j + 1][1] = sm.col[j + 1];
      }
      return;
    }
    const double x = (lane > j + 1 && lane < k) ? sm.col[lane] : 0.0;
    const double alpha = sm.col[j + 1];
    // x.x, x.ux, x.ub in one pass: v = x * scal + e_{j+1} gives v.u = scal (x.u) + u_{j+1}
    double xn2 = x * x, xux = x * ux, xub = x * ub, pad = 0.0;
    wave_sum4_dpp(xn2, xux, xub, pad);
    double tau = 0.0, beta = alpha, scal = 0.0;
    if (xn2 > 0.0) {  // dlarfg, with fp64 rcp/rsq refined to ~1 ulp
      const double a2 = fma(alpha, alpha, xn2);
      const double r = rsq64(a2);             // 1/|beta|
      beta = -copysign(a2 * r, alpha);
      tau = (beta - alpha) * -copysign(r, alpha);  // (beta - alpha) / beta
      scal = rcp64(alpha - beta);
    }
    if (lane == 0) {
      sm.tq[j + 1][1] = beta;
      sm.tau[j] = tau;
      f[F::SCAL + j] = scal;
    }
    if (tau == 0.0) return;  // H_j = I (uniform)
    // the factor keeps the unscaled, masked pivot column: a hit forms v as this step does
    if (lane > j && lane < KP) f[F::col(j) + lane - (j + 1)] = x;
    // v_i = x_i * scal (i > j+1), v_{j+1} = 1, 0 elsewhere
    const double v = lane == j + 1 ? 1.0 : x * scal;
    if (lane < KP) sm.vb[lane] = v;
    if (lane > j && lane < k) sm.u.reg[SM::hv_off(0) + j * (k - 1) - j * (j - 1) / 2 + lane - (j + 1)] = v;
    const double s2 = fma(scal, xux, readlane_f64(ux, j + 1));  // v . ux
    const double s3 = fma(scal, xub, readlane_f64(ub, j + 1));  // v . ub
    ux = fma(-tau * s2, v, ux);
    ub = fma(-tau * s3, v, ub);
    __syncthreads();
    // partials of A v (block rows >= J only: v vanishes above)
    double s1p = 0.0;  // this lane's share of v^T A v
    double pp = 0.0;
    double *pb = &sm.u.reg[SM::pb_base(J)] - J * SM::PLD;  // pb[R * PLD + col], R >= J
#pragma unroll
    for (int it = 0; it < NBL; ++it) {
      if (lane + 64 * it < NBLK && bi[it] >= J) {
        double vi[4], vj[4];
        ld4(&sm.vb[4 * bi[it]], vi);
        ld4(&sm.vb[4 * bj[it]], vj);
        double pr[4], pc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pr[r] = A[it][4 * r] * vj[0];
#pragma unroll
          for (int q = 1; q < 4; ++q) pr[r] = fma(A[it][4 * r + q], vj[q], pr[r]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          pc[q] = A[it][q] * vi[0];
#pragma unroll
          for (int r = 1; r < 4; ++r) pc[q] = fma(A[it][4 * r + q], vi[r], pc[q]);
        }
        double sp = vi[0] * pr[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) sp = fma(vi[r], pr[r], sp);
        double *dst = pb + bi[it] * SM::PLD + 4 * bj[it];
        *reinterpret_cast<double2 *>(dst) = make_double2(pr[0], pr[1]);
        *reinterpret_cast<double2 *>(dst + 2) = make_double2(pr[2], pr[3]);
        if (bi[it] != bj[it]) {
          if (bj[it] >= J) {
            double *dt = pb + bj[it] * SM::PLD + 4 * bi[it];
            *reinterpret_cast<double2 *>(dt) = make_double2(pc[0], pc[1]);
            *reinterpret_cast<double2 *>(dt + 2) = make_double2(pc[2], pc[3]);
          }
          sp = sp + sp;  // the transposed block contributes v_j^T B^T v_i = v_i^T B v_j
        }
        s1p += sp;
      }
    }
    const double s1 = tau * wave_sum_dpp(s1p);  // p . v with p = tau A v
    __syncthreads();
    if (lane < KP && lane > j) {
      const double *prow = pb + (lane >> 2) * SM::PLD + (lane & 3);
      pp = prow[0];
#pragma unroll
      for (int cb = 1; cb < SM::NB; ++cb) pp += prow[4 * cb];
    }
    const double p = (lane > j && lane < k) ? tau * pp : 0.0;
    const double w = fma(-0.5 * tau * s1, v, p);  // w = p - (tau/2)(p.v) v
    if (lane < KP) sm.wb[lane] = w;
    __syncthreads();
    // A <- A - v w^T - w v^T (rows and columns <= j are untouched: v, w vanish there)
#pragma unroll
    for (int it = 0; it < NBL; ++it) {
      if (lane + 64 * it < NBLK && bi[it] >= J) {
        double vi[4], vj[4], wi[4], wj[4];
        ld4(&sm.vb[4 * bi[it]], vi);
        ld4(&sm.vb[4 * bj[it]], vj);
        ld4(&sm.wb[4 * bi[it]], wi);
        ld4(&sm.wb[4 * bj[it]], wj);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            A[it][4 * r + q] = fma(-vi[r], wj[q], fma(-wi[r], vj[q], A[it][4 * r + q]));
      }
    }
  };
  // unrolled by the block width, so that the pivot column's registers are known statically
  using std::integral_constant;
  for (int j = 0; j < k; j += 4) {
    step(j, integral_constant<int, 0>{}, acc);
    if (j + 1 < k) step(j + 1, integral_constant<int, 1>{}, acc);
    if (j + 2 < k) step(j + 2, integral_constant<int, 2>{}, acc);
    if (j + 3 < k) step(j + 3, integral_constant<int, 3>{}, acc);
  }
  if (lane < KP) {
    sm.tq[lane][2] = ub;
    sm.tq[lane][3] = ux;
  }
  __syncthreads();
  if (lane < KP) {  // T, Q^T b1 and tau as the loop left them (the padding's rows included)
    f[F::D + lane] = sm.tq[lane][0];
    f[F::C + lane] = sm.tq[lane][1];
    f[F::U1 + lane] = ub;
    f[F::TAU + lane] = sm.tau[lane];
  }
  // the quadrature level, from the spectrum bound M / m = trace / inflat - (k - 1)
  const double ratio = trace / (double)c.inflat - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }
  tq_wave_finish<KP>(sm, c, slab, gi, lane, k, P, xbl, xb_mean, ratio, level, dec, ptot, info);
}

// One point per wavefront from its WaveFactor.  info[gi].x is the accepted count the fill left
// (restored by the host); the flags and alphas are this call's.
template <int KP>
__global__ void __launch_bounds__(64, TqOccupancy<KP>::kWaves)
solve_tq_wave_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                            const double *__restrict__ fac, int2 *__restrict__ info) {
  static_assert(KP % 8 == 0 && KP > 40 && KP <= 64, "KP");
  using SM = TqSmem<KP>;
  using F = WaveFactor<KP>;
  constexpr int NS = KP - 2;  // steps with a reflector at k = KP
  __shared__ SM sm;

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= npts) return;
  const int lane = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var and info stay as they are

  const long long P = wave_point_index(slab, g0 + gi);
  float xbl = 0.0f;
  if (lane < k) xbl = slab.var[P + slab.L * lane];
  // (x' is the first value the chain needs: its load goes out first, not behind the factor's,
  // whose addresses are ready sooner)
  __builtin_amdgcn_sched_barrier(0);
  // the factor, in the order of first use: the steps' scalars, the columns, then what only
  // the solve reads.  Lane i holds row i of every column.  The loads are unconditional, from
  // one lane base with a constant offset each (a load under a lane mask is a branch of its
  // own, and the waits behind such branches come out as vmcnt(0): the first step would wait
  // for the whole factor): a lane above the column's rows reads a word further up in the
  // point's own factor, lanes past KP read row KP - 1, and the mask is applied at the use.
  const auto *f = gptr(fac + (long long)gi * F::WORDS) + (lane < KP ? lane : KP - 1);
  // (the scheduler is free to reorder independent loads, and a step's wait counts the loads
  // issued after its own: the barriers keep the order of first use)
  const double tauv = f[F::TAU], scalv = f[F::SCAL];
  __builtin_amdgcn_sched_barrier(0);
  double x[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    static_assert(F::COL >= NS, "a lane above row j + 1 stays inside the factor");
    x[j] = f[F::col(j) - (j + 1)];
    __builtin_amdgcn_sched_barrier(0);
  }
  const double dv = f[F::D], cv = f[F::C], u1 = f[F::U1];
  __builtin_amdgcn_sched_barrier(0);

  asm volatile("" : "+v"(xbl));  // the wait for xbl alone, ahead of the loop that sums it
  const double xb_mean = wave_xb_mean(xbl, k, c.nmember_inv);
  double ux = (lane < k) ? (double)xbl - xb_mean : 0.0;  // x', becomes Q^T x'
  // ---- the x' half of every step (solve_tq_kernel's step: the same expressions) -----------
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    // (one nested test, no break: the loop unrolls, so that x[] stays in registers)
    const double tau = readlane_f64(tauv, j), scal = readlane_f64(scalv, j);
    // not the trailing 2x2 block, and not H_j = I (both uniform)
    if (j < k - 2 && !(tau == 0.0)) {
      // the fill's slot of wave_sum4_dpp (the sum's bits do not depend on it; a NaN's might)
      const double xj = (lane > j + 1 && lane < k) ? x[j] : 0.0;  // the fill's masked x
      double p0 = 0.0, xux = xj * ux, p2 = 0.0, p3 = 0.0;
      wave_sum4_dpp(p0, xux, p2, p3);
      const double v = lane == j + 1 ? 1.0 : xj * scal;
      if (lane > j && lane < k) sm.u.reg[j * (k - 1) - j * (j - 1) / 2 + lane - (j + 1)] = v;
      const double s2 = fma(scal, xux, readlane_f64(ux, j + 1));  // v . ux
      ux = fma(-tau * s2, v, ux);
    }
  }
  // sm.tq and sm.tau as the single kernel's loop leaves them
  if (lane < KP) {
    sm.tq[lane][0] = dv;
    sm.tq[lane][1] = cv;
    sm.tq[lane][2] = u1;
    sm.tq[lane][3] = ux;
    sm.tau[lane] = tauv;
  }
  if (lane == 0) sm.tq[KP][1] = 0.0;
  // trace A = sum of T's live diagonal, added in the steps' order
  double trace = 0.0;
  for (int j = 0; j < k; ++j) trace += readlane_f64(dv, j);
  __syncthreads();
  // the quadrature level, from the spectrum bound M / m = trace / inflat - (k - 1)
  const double ratio = trace / (double)c.inflat - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }
  tq_wave_finish<KP>(sm, c, slab, gi, lane, k, P, xbl, xb_mean, ratio, level, dec, ptot, info);
}

hipError_t launch_fill_tq_wave(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                               SlabDev slab, long long g0, int npts, const int *nbr_cnt,
                               const int *nbr_idx, int2 *info, double *fac) {
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || !fac || !info) return hipErrorInvalidValue;
#define CWBL_TQW_CASE(K)                                                                     \
  case K:                                                                                    \
    hipLaunchKernelGGL((fill_tq_wave_kernel<K>), dim3(npts), dim3(64), 0, s, trees, c, slab, \
                       g0, npts, nbr_cnt, nbr_idx, info, fac);                               \
    return hipGetLastError();
  switch (kp) {
    CWBL_TQW_CASE(48)
    CWBL_TQW_CASE(56)
    CWBL_TQW_CASE(64)
    default:
      return hipErrorInvalidValue;
  }
#undef CWBL_TQW_CASE
}

hipError_t launch_solve_tq_wave_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                       long long g0, int npts, const double *fac, int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || !fac || !info) return hipErrorInvalidValue;
#define CWBL_TQW_CASE(K)                                                                      \
  case K:                                                                                     \
    hipLaunchKernelGGL((solve_tq_wave_factor_kernel<K>), dim3(npts), dim3(64), 0, s, c, slab, \
                       g0, npts, fac, info);                                                  \
    return hipGetLastError();
  switch (kp) {
    CWBL_TQW_CASE(48)
    CWBL_TQW_CASE(56)
    CWBL_TQW_CASE(64)
    default:
      return hipErrorInvalidValue;
  }
#undef CWBL_TQW_CASE
}

}  // namespace cwbl
