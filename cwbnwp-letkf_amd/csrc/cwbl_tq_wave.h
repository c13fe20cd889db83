// cwbl_tq_wave.h — what the kernels that solve one point per wavefront from a WaveFactor<KP>
// share (cwbl_tq_wave.hip: the factor cache's fill and hit kernels, CWBL_OPT_WAVE_REUSE;
// cwbl_tq_wave_column.hip: the level kernel of a column-shared call, CWBL_OPT_COLUMN_FACTOR;
// cwbl_tq_wave_column_all.hip: its all-levels form, CWBL_OPT_COLUMN_REUSE):
// tq_wave_finish (solve_tq_kernel's text from the quadrature to the stores), the point
// index, the fp32 background mean and tq_wave_factor_levels, the all-levels kernel's body.  As a
// header the text leaves the instruction streams of cwbl_tq_wave.hip's and
// cwbl_tq_wave_column.hip's kernels as they were (profiles/column_factor.txt,
// profiles/column_reuse.txt).
#pragma once

#include "cwbl_tq_common.h"

namespace cwbl {

// What follows the Householder loop in solve_tq_kernel, from the quadrature to the stores:
// sm.tq, sm.tau and the packed vectors in sm.u.reg[0, NHV) are as the loop leaves them.  The
// caller has chosen the quadrature level as solve_tq_kernel does (ratio = trace / inflat -
// (k - 1), level and dec from its decade loop): per point in the factor cache's kernels, once
// per column in the level kernel, whose levels share the trace.
template <int KP>
__device__ __forceinline__ void tq_wave_finish(TqSmem<KP> &sm, const SolveConsts &c,
                                               const SlabDev &slab, int gi, int lane, int k,
                                               long long P, float xbl, double xb_mean,
                                               double ratio, int level, double dec, int ptot,
                                               int2 *__restrict__ info) {
  using SM = TqSmem<KP>;
  constexpr int H = KP / 2;
  double *Ym = &sm.u.reg[SM::NHV], *Zm = Ym + KP;
  // ---- T^-1/2 u2 by quadrature, u1^T T^-1 u2 exactly --------------------------------------
  const double m = (double)c.inflat;
  const int node = lane & 31, side = lane >> 5;
  const int npass = quad_passes(level);
  const double2 *rule = quad_rule(c.quad_r, npass == 1 ? 4 : 8, level);
  const unsigned q0 = side ? (KP - 1) * 32u : 0u, dirb = side ? (unsigned)-32 : 32u;
  const unsigned csb = side ? 40u : 8u;
  double *ym = Ym + side * H, *zm = Zm + side * H;
  for (int pass = 0; pass < npass; ++pass) {
    const bool exact = pass == 0 && node == 31;
    double sigma = 0.0, omega = 0.0;
    if (!exact) {
      const double2 tw = rule[31 * pass + node];
      sigma = m * tw.x;
      omega = sqrt(m) * tw.y;
    }
    double hh[H], mm[H];
    double dl = lds_at(sm.tq, q0) + sigma;
    double gt = lds_at(sm.tq, q0 + 24);
    double rdl = rcp64(dl);
#pragma unroll
    for (int t = 1; t < H; ++t) {
      const unsigned o = opaque_after(q0, dl) + dirb * (unsigned)t;
      const double ct = lds_at(sm.tq, o + csb);
      const double l = ct * rdl;
      hh[t - 1] = gt * rdl;
      mm[t - 1] = l;  // = c_t / dl_{t-1}
      asm volatile("" : "+v"(hh[t - 1]));  // materialise now: g_{t-1} and 1/dl_{t-1} die here
      dl = fma(-l, ct, lds_at(sm.tq, o) + sigma);
      gt = fma(-l, gt, lds_at(sm.tq, o + 24));
      rdl = rcp64(dl);
      __builtin_amdgcn_sched_barrier(0);  // keep the recurrence in order: bounded live ranges
    }
    // meeting rows H-1 (top) and H (bottom): 2x2 solve with the partner lane's pivot
    const double cm = sm.tq[H][1];
    const double dlo = __shfl_xor(dl, 32, 64), go = __shfl_xor(gt, 32, 64);
    double xv = (gt * dlo - cm * go) / fma(dl, dlo, -cm * cm);
    {
      const double ys = half_sum_dpp(omega * xv);
      if (node == 0) ym[H - 1] = pass ? ym[H - 1] + ys : ys;
      if (exact) zm[H - 1] = xv;
    }
#pragma unroll
    for (int t = H - 2; t >= 0; --t) {
      xv = fma(-mm[t], xv, hh[t]);
      const double ys = half_sum_dpp(omega * xv);
      if (node == 0) ym[t] = pass ? ym[t] + ys : ys;
      if (exact) zm[t] = xv;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();
  const int wi = lane < H ? lane : H + (KP - 1 - lane);  // walk slot of row `lane`
  const double zl = lane < KP ? Zm[wi] : 0.0;
  double yl = lane < KP ? Ym[wi] : 0.0;
  const double d = wave_sum_dpp(lane < KP ? sm.tq[lane][2] * zl : 0.0);  // u1 . T^-1 u2

  // ---- back-transform: y <- Q y = H_0 H_1 ... H_{k-3} y, two reflectors per reduction ----
  auto hvec = [&](int j) {
    const int off = j * (k - 1) - j * (j - 1) / 2;
    return (lane > j && lane < k) ? sm.u.reg[off + lane - (j + 1)] : 0.0;
  };
  int j = k - 3;
  for (; j >= 1; j -= 2) {
    const double t1 = sm.tau[j], t0 = sm.tau[j - 1];
    // a reflector with tau = 0 was never stored (H = I): use a zero vector
    const double v1 = t1 == 0.0 ? 0.0 : hvec(j), v0 = t0 == 0.0 ? 0.0 : hvec(j - 1);
    double a1 = v1 * yl, b0 = v0 * yl, c01 = v0 * v1, pad = 0.0;
    wave_sum4_dpp(a1, b0, c01, pad);
    yl = fma(-t1 * a1, v1, yl);
    yl = fma(-t0 * fma(-t1 * a1, c01, b0), v0, yl);
  }
  if (j == 0 && sm.tau[0] != 0.0) {
    const double v0 = hvec(0);
    const double s0 = wave_sum_dpp(v0 * yl);
    yl = fma(-sm.tau[0] * s0, v0, yl);
  }
  const double sk = sqrt((double)(k - 1));
  // analysis of member `lane` (xa = wbar, :675-679); fp32 from here on, in registers
  float xal = lane < KP ? (float)(xb_mean + (d + sk * yl)) : 0.0f;

  // ---- RTPP / RTPS (:684-698), fp32 in the reference's order -------------------------
  auto seq_sum = [&](float x) {
    float s = 0.0f;
    for (int mm = 0; mm < k; ++mm) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), mm));
    return s;
  };
  if (c.use_rtpp || c.use_rtps) {
    const float xa_mean = seq_sum(xal) * c.nmember_inv;
    const double xpl = lane < k ? (double)xbl - xb_mean : 0.0;
    float xap = 0.0f;
    if (lane < k) {
      xap = xal - xa_mean;
      if (c.use_rtpp)
        xap = (float)((double)((1.0f - c.rtpp_alpha) * xap) + (double)c.rtpp_alpha * xpl);
    }
    if (c.use_rtps) {
      double d8 = 0.0;
      for (int mm = 0; mm < k; ++mm) {
        const double xp = readlane_f64(xpl, mm);
        d8 = d8 + xp * xp;
      }
      const float xb_std = (float)d8;
      const float xa_std = seq_sum(xap * xap);
      xap = xap * (c.rtps_alpha * sqrtf(xb_std / xa_std) - c.rtps_alpha + 1.0f);
    }
    xal = xa_mean + xap;
  }

  if (lane < k) slab.var[P + slab.L * lane] = xal;
  // info.y: decade of the quadrature rule (negative when M/m exceeds the last table)
  if (lane == 0 && info) info[gi] = make_int2(ptot, ratio > dec ? -level : level);
}

// var index of member 0 of point g
__device__ __forceinline__ long long wave_point_index(const SlabDev &slab, long long g) {
  const int i = (int)(g % slab.ix_lim);
  const long long r = g / slab.ix_lim;
  const int j = (int)(r % slab.iy_lim);
  const int kz = (int)(r / slab.iy_lim);
  return i + (long long)slab.nx * (j + (long long)slab.ny * kz);
}

// xb_mean = sum(xb) * nmember_inv in fp32 (:671), sequential like the reference
__device__ __forceinline__ double wave_xb_mean(float xbl, int k, float nmember_inv) {
  float s = 0.0f;
  for (int mm = 0; mm < k; ++mm)
    s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xbl), mm));
  return (double)(s * nmember_inv);
}

// The body of a level kernel of a column-shared call, with the first level as an argument: the
// levels kzf + lw blockIdx.y .. of column blockIdx.x (through xcd_remap) from the WaveFactor<KP>
// at fac + gi WORDS.  cwbl_tq_wave_column_all.hip calls it with kzf = 0 (every level of a column
// whose factor the column cache kept, CWBL_OPT_COLUMN_REUSE).  It is the text of
// solve_tq_wave_factor_column_kernel (cwbl_tq_wave_column.hip), which starts at level 1 and
// keeps its own copy: as a caller of this function that kernel compiles to another schedule
// (profiles/column_reuse.txt), and its assembly is not to change.  sm is the workgroup's own.
// Per level the text is solve_tq_wave_factor_kernel's replay and tq_wave_finish; see
// cwbl_tq_wave_column.hip for what is done once per wavefront and for the redefinitions that
// keep a level's text inside the loop.  info is read only.
template <int KP>
__device__ __forceinline__ void tq_wave_factor_levels(TqSmem<KP> &sm, const SolveConsts &c,
                                                      const SlabDev &slab, long long g0, int ncol,
                                                      int nz, int lw, int kzf,
                                                      const double *__restrict__ fac,
                                                      const int2 *__restrict__ info) {
  static_assert(KP % 8 == 0 && KP > 40 && KP <= 64, "KP");
  using F = WaveFactor<KP>;
  constexpr int NS = KP - 2;  // steps with a reflector at k = KP

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= ncol) return;
  const int kz0 = kzf + (int)blockIdx.y * lw, kz1 = min(nz, kz0 + lw);  // levels [kz0, kz1)
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

}  // namespace cwbl
