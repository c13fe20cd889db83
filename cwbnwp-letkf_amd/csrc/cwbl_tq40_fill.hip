// cwbl_tq40_fill.hip — the record cache's kernel pair (CWBL_OPT_FACTOR_REUSE): the cached
// batches keep the factor A = Q T Q^T of every point instead of its record (A, b1).
//
//   fill_tq40_factor_kernel<KP>   a cache fill: solve_tq40_multi_kernel's b1-only
//                                 tridiagonalisation of the record, then the factor
//                                 (FactorRecord, cwbl_internal.h) goes out over the record it
//                                 came from, the steps' beta and tau to the point's FactorAux
//                                 entry, and the call's variable is solved from it;
//   solve_tq40_factor_kernel<KP>  a cache hit: loads the factor where the multi kernel keeps
//                                 its reflectors (phase 1: sm.pv, phase 2: the registers of the
//                                 columns they eliminated) and T's off-diagonal and the taus
//                                 where it keeps those (sm.tq, sm.tau), and solves the call's
//                                 variable.  No O(k^3) work and no dlarfg: the kernel streams
//                                 6880 + 640 B per point;
//                                 (cwbl_tq40_hit_merge.hip has the same hit for several cached
//                                 batches in one launch; the text the three kernels share is
//                                 cwbl_tq40_factor.h).
//
// The factor is a function of the record alone, and both kernels run the same text
// (tq40_factor_solve) on it: the multi kernel's replay of the reflectors on x', then the
// trace, the level, the wave's rounds, the quadrature, d, the back-transform and the RTPP/RTPS
// epilogue.  Every floating-point expression is one solve_tq40_kernel evaluates on the same
// bits, so a fill or a hit equals solve_tq40_kernel on the record bit for bit:
//   - x is kept unscaled and masked (0 on the rows <= j + 1 and >= k), as the step formed it;
//   - beta, tau and scal are kept as the step's dlarfg returned them (its xx == 0 branch and
//     NaNs included): the hit stores what it loaded, nothing is derived again.  scal lies at
//     row j + 1 of the factor's column j, which is the lane (phase 2) or, the column's first
//     word, the address (phase 1) that the replay reads it from.
//
// In place: a wave is the only reader of its four records and has loaded them entirely
// (tq40_load_record; every loaded word feeds step 0) before the factor's first store; lanes
// past npts only ever read the spare record and store nothing.  The FactorAux entries are a
// buffer of their own: plain stores from the valid lanes.
#include "cwbl_tq40_factor.h"

namespace cwbl {

// ---- the fill: record -> factor (in place) and the call's variable ---------------------------
template <int KP>
__global__ void __launch_bounds__(64, 2)
fill_tq40_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                        double *__restrict__ ws, double *__restrict__ aux,
                        int2 *__restrict__ info) {
  using LY = Tq40Layout<KP>;
  using FR = FactorRecord<KP>;
  using FA = FactorAux<KP>;
  constexpr int J0 = LY::J0, KT = LY::KT, NS = LY::NS;
  using SM = Tq40Smem<KP>;
  __shared__ SM sm;

  const int lane = threadIdx.x, q = lane >> 4, l = lane & 15;
  // the order of solve_tq40_kernel: XCD by XCD, each XCD's chunk from its end
  const int g4 = xcd_remap_rev(blockIdx.x, gridDim.x);
  const int gi = 4 * g4 + q;
  const bool valid = gi < npts;
  const int k = c.k;
  const int ptot = valid ? info[gi].x : 0;

  // ---- A and b1 from the record ---------------------------------------------------------------
  double A[NS][KP];  // slot rows, all columns
  double Pb[J0];     // prefix block row l (lanes >= J0 hold row 0's copy, never used)
  const bool pre = l < J0;
  double ubP, ub[NS];
  tq40_load_record<KP>(ws, g4, q, l, valid, npts, A, Pb, ubP, ub);

  // ---- phase 1: Householder steps 0 .. J0-1 with the prefix block (b1 only) ---------------
  // (twin: solve_tq40_multi_kernel's phase 1 and phase 2)
  sfor<J0>([&](auto jj) {
    constexpr int j = decltype(jj)::value, J1 = j + 1;
    const double dj = rbcast<j>(Pb[j]);  // A(j,j): final diagonal of T
    // alpha = A(j+1, j): prefix row j+1, or slot 0 lane 0 (row J0) at the last step
    double alpha, u1a;
    if constexpr (J1 < J0) {
      alpha = rbcast<J1>(Pb[j]);
      u1a = rbcast<J1>(ubP);
    } else {
      alpha = rbcast<0>(A[0][j]);
      u1a = rbcast<0>(ub[0]);
    }
    // x: column j below row j + 1 (rows < k)
    const double xP = (pre && l > J1 && l < k) ? Pb[j] : 0.0;
    double x[NS];
    double xx = xP * xP, xb = xP * ubP;
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      const int i = J0 + l + 16 * r;
      x[r] = (i > J1 && i < k) ? A[r][j] : 0.0;
      xx = fma(x[r], x[r], xx);
      xb = fma(x[r], ub[r], xb);
    });
    rsum16x2(xx, xb);
    auto src_of = [&](auto cc, const double &vp, const double (&vs)[NS]) -> const double & {
      constexpr int col = decltype(cc)::value;
      if constexpr (col < J0) return vp;
      else return vs[(col - J0) / 16];
    };
    auto lane_of = [](int col) { return col < J0 ? col : (col - J0) % 16; };
    const Refl h = dlarfg(alpha, xx);
    // every lane of the row writes the same value (no divergent branch in the step)
    sm.tq[q][j][0] = dj;
    sm.tq[q][J1][1] = h.beta;
    sm.tau[q][j] = h.tau;
    const double tau = h.tau;
    // v: 1 at row j + 1, x * scal below
    const double xsP = xP * h.scal;
    double vP = (pre && l == J1) ? 1.0 : xsP;
    double v[NS];
    // the reflector is final: x goes to LDS UNSCALED (sm.pv[q][j]: word 0 takes the step's
    // scal, word 1 is the dump word of prefix rows 0, 1 and the lanes >= J0, whose x is 0)
    sm.pv[q][j][(pre && l > 1) ? l : 1] = xP;
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      const double xs = x[r] * h.scal;
      if constexpr (J1 == J0 && r == 0) v[r] = l == 0 ? 1.0 : xs;
      else v[r] = xs;
      sm.pv[q][j][J0 + l + 16 * r] = x[r];
    });
    sm.pv[q][j][0] = h.scal;
    const double s3 = fma(h.scal, xb, u1a);  // v . b1
    ubP = fma(-tau * s3, vP, ubP);
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      ub[r] = fma(-tau * s3, v[r], ub[r]);
    });
    dpp_pin(vP);
    sfor<NS>([&](auto rr) { dpp_pin(v[decltype(rr)::value]); });
    // A v: slot rows over columns j+1 .. KP-1; prefix rows = their block part + the column
    // sums over the slot rows (A(i, c) = A(c, i) for c >= J0)
    double pa[kNA][NS], pP = 0.0;
    sfor<kNA * NS>([&](auto ii) { pa[decltype(ii)::value / NS][decltype(ii)::value % NS] = 0.0; });
    sfor<KP - J1>([&](auto cc) {
      constexpr int col = J1 + decltype(cc)::value;
      constexpr int LC = lane_of(col);
      const double &vs = src_of(std::integral_constant<int, col>{}, vP, v);
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        constexpr int a = (col - J1) % kNA;
        pa[a][r] = fmac_row<LC>(pa[a][r], vs, A[r][col]);
      });
      if constexpr (col < J0) pP = fmac_row<LC>(pP, vs, Pb[col]);
    });
    if constexpr (J1 < J0) {  // prefix rows j+1 .. J0-1: column sums of the slots
      // (in chunks of up to three: seven sums at once spill)
      constexpr int NC = J0 - J1, CH = 3;
      sfor<(NC + CH - 1) / CH>([&](auto kk) {
        constexpr int c0 = J1 + CH * decltype(kk)::value;
        constexpr int n = J0 - c0 < CH ? J0 - c0 : CH;
        double cs[n];
        sfor<n>([&](auto cc) {
          constexpr int col = c0 + decltype(cc)::value;
          double s = 0.0;
          sfor<NS>([&](auto rr) {
            constexpr int r = decltype(rr)::value;
            s = fma(A[r][col], v[r], s);
          });
          cs[decltype(cc)::value] = s;
        });
        rsum16xN(cs);
        sfor<n>([&](auto cc) {
          constexpr int col = c0 + decltype(cc)::value;
          pP += l == col ? cs[decltype(cc)::value] : 0.0;
        });
      });
    }
    double pp[NS];
    double sp = vP * pP;  // rows <= j: v = 0
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      pp[r] = acc_sum(pa, r);
      sp = fma(v[r], pp[r], sp);
    });
    const double s1 = tau * rsum16(sp);  // v^T (tau A v)
    const double wP = fma(-0.5 * tau * s1, vP, tau * pP);
    double wv[NS];
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      wv[r] = fma(-0.5 * tau * s1, v[r], tau * pp[r]);
    });
    // A <- A - v w^T - w v^T: slot rows over columns j+1 .. KP-1, the prefix block over
    // columns j+1 .. J0-1 (v renamed first, as in solve_tq40_kernel)
    double wPp = wP;
    dpp_pin(wPp);
    sfor<NS>([&](auto rr) { dpp_pin(wv[decltype(rr)::value]); });
    sfor<(KP - J1 + kUG - 1) / kUG>([&](auto pp) {
      constexpr int c0 = J1 + kUG * decltype(pp)::value;
      sfor<2>([&](auto hh) {  // hh = 0: A - wv v_c; hh = 1: - v w_c (the reference's order)
        constexpr int h = decltype(hh)::value;
        sfor<kUG>([&](auto ee) {
          constexpr int col = c0 + decltype(ee)::value;
          if constexpr (col < KP) {
            constexpr int LC = lane_of(col);
            const double &vs = src_of(std::integral_constant<int, col>{}, vP, v);
            const double &ws = src_of(std::integral_constant<int, col>{}, wPp, wv);
            sfor<NS>([&](auto rr) {
              constexpr int r = decltype(rr)::value;
              if constexpr (h == 0) A[r][col] = fnmac_row<LC>(A[r][col], vs, wv[r]);
              else A[r][col] = fnmac_row<LC>(A[r][col], ws, v[r]);
            });
            if constexpr (col < J0) {
              if constexpr (h == 0) Pb[col] = fnmac_row<LC>(Pb[col], vs, wPp);
              else Pb[col] = fnmac_row<LC>(Pb[col], ws, vP);
            }
          }
        });
      });
    });
  });
  // a (one-wave) workgroup barrier: a fence the scheduler does not move phase 2 across
  __syncthreads();
  // the prefix rows of Q^T b1 are final (later reflectors vanish there)
  if (pre) sm.tq[q][l][2] = ubP;

  // ---- phase 2: steps J0 .. KP-3 on the trailing rows (b1 only) ---------------------------
  // Steps j >= k - 2 (k < KP) are exact no-ops, as in solve_tq40_kernel.
  sfor<KT>([&](auto jj) {
    constexpr int jl = decltype(jj)::value, j = J0 + jl;
    constexpr int RJ = jl / 16, LJ = jl % 16;
    const double dj = rbcast<LJ>(A[RJ][j]);  // A(j,j): final diagonal of T
    if constexpr (jl + 2 < KT) {
      constexpr int J1 = jl + 1, R1 = J1 / 16, L1 = J1 % 16;
      const double alpha = rbcast<L1>(A[R1][j]);
      double x[NS], xx = 0.0, xb = 0.0;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 > J1) {
          const int i = J0 + l + 16 * r;
          x[r] = (i > j + 1 && i < k) ? A[r][j] : 0.0;
          xx = fma(x[r], x[r], xx);
          xb = fma(x[r], ub[r], xb);
        } else {
          x[r] = 0.0;
        }
      });
      rsum16x2(xx, xb);
      const Refl h = dlarfg(alpha, xx);
      const double tau = h.tau;
      sm.tq[q][j][0] = dj;
      sm.tq[q][j + 1][1] = h.beta;
      sm.tau[q][j] = tau;
      double v[NS];
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int t = l + 16 * r;
        const double xs = x[r] * h.scal;
        v[r] = t == J1 ? 1.0 : xs;
        // the reflector stays in column j's registers UNSCALED (rows > j + 1; 0 above), and
        // the step's scal takes row j + 1's known zero
        if constexpr (r == R1) A[r][j] = t == J1 ? h.scal : x[r];
        else if constexpr (16 * r + 15 > J1) A[r][j] = x[r];
      });
      const double s3 = fma(h.scal, xb, rbcast<L1>(ub[R1]));  // v . b1
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        ub[r] = fma(-tau * s3, v[r], ub[r]);
      });
      // A v over the trailing columns (v vanishes at columns <= j), column by column so
      // that one broadcast v_c is live at a time
      double pa[kNA][NS];
      sfor<kNA * NS>([&](auto ii) { pa[decltype(ii)::value / NS][decltype(ii)::value % NS] = 0.0; });
      sfor<NS>([&](auto rr) { dpp_pin(v[decltype(rr)::value]); });
      sfor<KT - J1>([&](auto cc) {
        constexpr int cl = J1 + decltype(cc)::value;
        sfor<NS>([&](auto rr) {
          constexpr int r = decltype(rr)::value;
          if constexpr (16 * r + 15 > jl) {
            constexpr int a = (cl - J1) % kNA;
            pa[a][r] = fmac_row<cl % 16>(pa[a][r], v[cl / 16], A[r][J0 + cl]);
          }
        });
      });
      double pp[NS], sp = 0.0;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        pp[r] = acc_sum(pa, r);
        if constexpr (16 * r + 15 > jl) sp = fma(v[r], pp[r], sp);  // rows <= j: v = 0
      });
      const double s1 = tau * rsum16(sp);  // v^T (tau A v)
      double wv[NS];
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        wv[r] = fma(-0.5 * tau * s1, v[r], tau * pp[r]);
      });
      // A <- A - v w^T - w v^T on the trailing rows and columns
      sfor<NS>([&](auto rr) { dpp_pin(wv[decltype(rr)::value]); });
      sfor<(KT - J1 + kUG - 1) / kUG>([&](auto pp) {
        constexpr int c0 = J1 + kUG * decltype(pp)::value;
        sfor<2>([&](auto hh) {
          constexpr int h = decltype(hh)::value;
          sfor<kUG>([&](auto ee) {
            constexpr int cl = c0 + decltype(ee)::value;
            if constexpr (cl < KT) {
              sfor<NS>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                if constexpr (16 * r + 15 > jl) {
                  if constexpr (h == 0)
                    A[r][J0 + cl] = fnmac_row<cl % 16>(A[r][J0 + cl], v[cl / 16], wv[r]);
                  else
                    A[r][J0 + cl] = fnmac_row<cl % 16>(A[r][J0 + cl], wv[cl / 16], v[r]);
                }
              });
            }
          });
        });
      });
    } else {  // the trailing 2x2: already tridiagonal (c(KP-2,KP-3) is step KP-3's beta)
      const double ej = rbcast<LJ>(A[RJ][j - 1]);
      sm.tq[q][j][0] = dj;
      if constexpr (jl == KT - 1) sm.tq[q][j][1] = ej;
    }
  });
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int i = J0 + l + 16 * r;
    sm.tq[q][i][2] = ub[r];
  });
  if (l == 0) {
    sm.tq[q][0][1] = 0.0;
    sm.tq[q][KP][1] = 0.0;
  }
  __syncthreads();

  // ---- the factor, over the record (valid lanes only; every record word is replaced) --------
  if (valid) {
    const unsigned wb = (unsigned)gi * (unsigned)FR::WORDS;
    auto st = [&](unsigned w, double x) { gst(ws, 8u * (wb + w), x); };
    sfor<(KP + 15) / 16>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      const int i = l + 16 * r;
      if (16 * r + 15 < KP || i < KP) st((unsigned)(FR::D + i), sm.tq[q][i][0]);
    });
    if (pre) st((unsigned)(FR::U1 + l), ubP);
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      st((unsigned)(FR::U1 + J0 + l + 16 * r), ub[r]);
    });
    sfor<J0>([&](auto jj) {  // phase 1's columns: scal (sm.pv's word 0) at row j + 1, x below
      constexpr int j = decltype(jj)::value, J1 = j + 1;
      const double *pj = sm.pv[q][j];
      if (pre && l >= J1) st((unsigned)(FR::col(j) + l - J1), pj[l == J1 ? 0 : l]);
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int i = J0 + l + 16 * r;
        if constexpr (J1 == J0 && r == 0) st((unsigned)(FR::col(j) + i - J1), pj[l == 0 ? 0 : i]);
        else st((unsigned)(FR::col(j) + i - J1), pj[i]);
      });
    });
    sfor<KT - 2>([&](auto jj) {  // phase 2's columns, as the registers hold them: scal at row
      constexpr int jl = decltype(jj)::value, j = J0 + jl, J1 = jl + 1;  // j + 1, x below
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 >= J1) {
          const int t = l + 16 * r;
          if (t >= J1) st((unsigned)(FR::col(j) + t - J1), A[r][j]);
        }
      });
    });
    if (l == 0) st((unsigned)FR::EL, 0.0);  // (unused: every record word is replaced)
    // the steps' beta and tau: the point's FactorAux
    const unsigned ab = (unsigned)gi * (unsigned)FA::WORDS;
    sfor<(KP + 15) / 16>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      const int i = l + 16 * r;
      if (16 * r + 15 < KP || i < KP) {
        gst(aux, 8u * (ab + (unsigned)(FA::B + i)), sm.tq[q][i][1]);
        // (steps KP-2 and KP-1 do not exist: sm.tau has nothing there)
        const double tj = sm.tau[q][i < KP - 2 ? i : 0];
        gst(aux, 8u * (ab + (unsigned)(FA::T + i)), i < KP - 2 ? tj : 0.0);
      }
    });
  }

  float xv[LY::NV];
  tq40_load_xb<KP>(slab, g0, valid, gi, l, k, xv);
  tq40_factor_solve<KP, false>(c, slab, sm, A, xv, g0, valid, ptot, gi, q, l, info);
}

template <int KP>
__global__ void __launch_bounds__(64, 2)
solve_tq40_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                         const double *__restrict__ ws, const double *__restrict__ aux,
                         int2 *__restrict__ info) {
  tq40_factor_hit<KP>(c, slab, g0, npts, ws, aux, info, blockIdx.x, gridDim.x);
}

hipError_t launch_fill_tq40_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   long long g0, int npts, double *ws, double *aux, int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad_r == nullptr || aux == nullptr || kp != kTq4KP) return hipErrorInvalidValue;
  const dim3 grid((npts + 3) / 4);
  hipLaunchKernelGGL((fill_tq40_factor_kernel<kTq4KP>), grid, dim3(64), 0, s, c, slab, g0, npts,
                     ws, aux, info);
  return hipGetLastError();
}

hipError_t launch_solve_tq40_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                    long long g0, int npts, const double *ws, const double *aux,
                                    int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad_r == nullptr || aux == nullptr || kp != kTq4KP) return hipErrorInvalidValue;
  const dim3 grid((npts + 3) / 4);
  hipLaunchKernelGGL((solve_tq40_factor_kernel<kTq4KP>), grid, dim3(64), 0, s, c, slab, g0, npts,
                     ws, aux, info);
  return hipGetLastError();
}

}  // namespace cwbl
