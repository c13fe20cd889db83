// cwbl_tq40_passes.h — tq40_passes<KP>: solve_tq40_kernel (cwbl_tq40.hip) for several x' that
// share one factor.  It is the whole body of solve_tq40_multi_kernel (cwbl_tq40_multi.hip: a
// pass is a variable of a group) and of solve_tq40_column_kernel (cwbl_tq40_column.hip: a pass
// is a level of the wave's range of a column); a policy at its edges says what the passes are.
//
// A = inflat I + Yb Yb^T, b1 = Yb d and therefore the factor A = Q T Q^T do not depend on the
// pass; only x' does.  solve_tq40_kernel applies every reflector on the fly to b1 and to x'.
// This body, with the same layout (four points per wavefront, one 16-lane DPP row per point,
// J0 prefix steps, the trailing 32 x 32 on full rows), runs the tridiagonalisation once per
// point carrying b1 only and keeps what a replay needs to repeat the x' half of each step bit
// for bit:
//
//   s2 = fma(scal, sum x ux, u2a) is formed from the UNSCALED masked pivot column x and the
//   step's scal, and v = x scal is the same multiply again.  So the reflectors are kept as x
//   (phase 1: pv in LDS, phase 2: the registers of the column they eliminated) and scal goes
//   where the column holds a known zero: pv[q][j][0] (rows <= j + 1 of a phase-1 column are
//   unused) and row j + 1 of column j in phase 2.
//
// A runtime loop over the passes then loads the point's background from the pass's var, forms
// x', replays the KP - 2 reflectors on it in step order (one dot, one row sum, one axpy per
// step), and runs solve_tq40_kernel's quadrature, back-transform and RTPP/RTPS epilogue with
// that pass's flags.  Every expression is the one solve_tq40_kernel evaluates (the project
// builds with -ffp-contract=off and the steps use explicit fma), so each pass's analysis
// equals solve_tq40_kernel's on the same record and under the same quadrature rule bit for
// bit.  The loop body is the same code for every pass: all register indices stay static.
//
// Shared with solve_tq40_kernel through cwbl_tq40_common.h: the layout constants and the
// shared-memory struct, the row sums, dlarfg, the point decode, the record load, the trace and
// the wave's quadrature rounds.  This file's own: the b1-only tridiagonalisation that keeps x
// and scal (its matvec and rank-2 update repeat cwbl_tq40.hip's phase 1 and phase 2, which
// carry x' as well and keep x scal), the replay, and the back-transform from x and scal.  The
// quadrature (level loop, round loop, d) and the RTPP/RTPS epilogue repeat cwbl_tq40.hip's
// text: as shared functions they cost the group kernel 2 % per launch at eight variables.
#pragma once

#include "cwbl_tq40_common.h"

#include <utility>

namespace cwbl {

// One pass: the var it analyses in place and its RTPP/RTPS flags and alphas
struct Tq40Pass {
  float *var;
  int use_rtpp, use_rtps;
  float rtpp_alpha, rtps_alpha;
};

// The passes policy of tq40_passes: passes first() .. last() - 1 in order, pass(i), and
// whether this wave stores the points' info.
//
// The variables of a group, each with its own flags (by-value tables in the kernel's arguments)
struct Tq40GroupPasses {
  const Tq40Vars &vars;
  __device__ __forceinline__ int first() const { return 0; }
  __device__ __forceinline__ int last() const { return vars.nvar; }
  __device__ __forceinline__ Tq40Pass pass(int iv) const {
    return {vars.var[iv], vars.use_rtpp[iv], vars.use_rtps[iv], vars.rtpp_alpha[iv],
            vars.rtps_alpha[iv]};
  }
  __device__ __forceinline__ bool writes_info() const { return true; }
};

// Levels [lw blockIdx.y, + lw) of the nz levels of a column: level kz's var is slab.var +
// nx ny kz (arithmetic, no pointer table, so nz has no cap), the flags and alphas are
// SolveConsts's, and the wave of the first range stores info
struct Tq40LevelPasses {
  const SolveConsts &c;
  const SlabDev &slab;
  int nz, lw;
  __device__ __forceinline__ int first() const { return (int)blockIdx.y * lw; }
  __device__ __forceinline__ int last() const { return min(first() + lw, nz); }
  __device__ __forceinline__ Tq40Pass pass(int kz) const {
    const long long nxy = (long long)slab.nx * slab.ny;  // var index step of a level
    return {slab.var + nxy * kz, c.use_rtpp, c.use_rtps, c.rtpp_alpha, c.rtps_alpha};
  }
  __device__ __forceinline__ bool writes_info() const { return blockIdx.y == 0; }
};

namespace {

// Two row sums (the steps' x.x and x.b1: rsum16x3 without the x' sum)
__device__ __forceinline__ void rsum16x2(double &a, double &b) {
  double ab[2] = {a, b};
  rsum16xN(ab);
  a = ab[0];
  b = ab[1];
}

// x, redefined in place: the compiler sees a new value, no instruction is emitted
__device__ __forceinline__ void touch(double &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ int touched(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ long long touched(long long x) {
  asm volatile("" : "+v"(x));
  return x;
}

}  // namespace

template <int KP, class Passes>
__device__ __forceinline__ void tq40_passes(const SolveConsts &c, const SlabDev &slab,
                                            const Passes &passes, long long g0, int npts,
                                            double *__restrict__ ws, int2 *__restrict__ info) {
  using LY = Tq40Layout<KP>;
  constexpr int J0 = LY::J0, KT = LY::KT, NS = LY::NS, NV = LY::NV, H = LY::H;
  using SM = Tq40Smem<KP>;
  __shared__ SM sm;

  const int lane = threadIdx.x, q = lane >> 4, l = lane & 15;
  // the order of solve_tq40_kernel: XCD by XCD, each XCD's chunk from its end
  const int g4 = xcd_remap_rev(blockIdx.x, gridDim.x);
  const int gi = 4 * g4 + q;
  const bool valid = gi < npts;
  const int k = c.k;
  const int ptot = valid ? info[gi].x : 0;
  auto vrow = [&](int vs) { return tq40_vrow<KP>(l, vs); };
  const long long P = tq40_var_index(slab, g0, valid ? gi : 0);  // var index of member 0

  // ---- A and b1 from the record ---------------------------------------------------------------
  double A[NS][KP];  // slot rows, all columns
  double Pb[J0];     // prefix block row l (lanes >= J0 hold row 0's copy, never used)
  const int lp = l < J0 ? l : 0;
  const bool pre = l < J0;
  double ubP, ub[NS];
  tq40_load_record<KP>(ws, g4, q, l, valid, npts, A, Pb, ubP, ub);

  // ---- phase 1: Householder steps 0 .. J0-1 with the prefix block (b1 only) ---------------
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
    // the reflector is final: x goes to LDS UNSCALED, for the replays and the back-transform
    // (sm.pv[q][j]: rows <= j + 1 of a column are unused, so word 0 takes the step's scal and
    // word 1 is the dump word of prefix rows 0, 1 and the lanes >= J0, whose x is 0), and
    // column j's registers are dead from here on
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
  const double trace = tq40_trace(sm, q, l, k);

  // ---- the quadrature rule of the point: T only, once ---------------------------------------
  // (twin: this level loop and the walk's LDS offsets below are solve_tq40_kernel's)
  const double m = (double)c.inflat;
  const double ratio = trace / m - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }
  const int R = tq40_wave_rounds(level);
  const int NQ = 8 * R - 1;  // (R is wave-uniform)
  const double2 *qtab = quad_rule(c.quad_r, R, level);
  const int side = l >> 3, n8 = l & 7;
  const double(*T)[4] = sm.tq[q];
  char *const smb = reinterpret_cast<char *>(&sm);
  auto lds = [&](unsigned off) { return *reinterpret_cast<const double *>(smb + off); };
  auto sts = [&](unsigned off, double v) { *reinterpret_cast<double *>(smb + off) = v; };
  const unsigned tq0 = (unsigned)(offsetof(SM, tq) + (size_t)q * sizeof(sm.tq[0])) +
                       (side ? (KP - 1) * 32u : 0u);   // row 0 of the walk
  const unsigned dirb = side ? (unsigned)-32 : 32u;   // next row of the walk
  const unsigned csb = side ? 40u : 8u;  // coupling with the previous row of the walk
  const unsigned qs0 = (unsigned)(offsetof(SM, qs) + (size_t)q * sizeof(sm.qs[0])) +
                       (side ? (KP - H) * 8u : (H - 1) * 8u);  // row H-1 of the walk
  const unsigned qz0 = (unsigned)(offsetof(SM, qz) + (size_t)q * sizeof(sm.qz[0]));
  const unsigned bdir = side ? 8u : (unsigned)-8;    // back-substitution: previous row
  const double sk = sqrt((double)(k - 1));
  // The kept columns, redefined in place through an empty asm: what the replay and the
  // back-transform derive from them (x scal, the scal broadcasts, the row j + 1 selects) is
  // the same for every pass, and hoisted out of the pass loop, or shared between the
  // replay and the back-transform across the quadrature, it would double the live registers
  auto touch_cols = [&]() {
    sfor<KT - 2>([&](auto jj) {
      constexpr int jl = decltype(jj)::value, J1 = jl + 1, R1 = J1 / 16;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 > J1 || r == R1) touch(A[r][J0 + jl]);
      });
    });
  };

  // ---- the passes ---------------------------------------------------------------------------
  const int ip0 = passes.first(), ip1 = passes.last();
#pragma unroll 1
  for (int ip = ip0; ip < ip1; ++ip) {
    const Tq40Pass pass = passes.pass(ip);
    float *__restrict__ const var = pass.var;
    const int use_rtpp = pass.use_rtpp, use_rtps = pass.use_rtps;
    const float rtpp_alpha = pass.rtpp_alpha, rtps_alpha = pass.rtps_alpha;

    // background of the point: member i = row i
    float xbl[NV];
    double xb_mean;
    {
      // (P, redefined: the member addresses are formed here, not kept across the loop)
      const long long Pl = touched(P);
      sfor<NV>([&](auto vv) {
        constexpr int vs = decltype(vv)::value;
        const int i = vrow(vs);
        const bool mem = valid && i < k;
        const float xv = var[Pl + slab.L * touched(mem ? i : 0)];  // branch-free: a valid address
        xbl[vs] = mem ? xv : 0.0f;
      });
      // sum(xb) * nmember_inv (:671)
      xb_mean = (double)(seq_sum_f32<KP>(xbl) * c.nmember_inv);
    }
    // x' (fp64, :671-672)
    double uxP = pre && l < k ? (double)xbl[0] - xb_mean : 0.0, ux[NS];
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      const int t = J0 + l + 16 * r;
      ux[r] = t < k ? (double)xbl[r + 1] - xb_mean : 0.0;
    });

    touch_cols();
    // ---- replay: x' <- Q^T x', the x' half of every step of solve_tq40_kernel ------------
    sfor<J0>([&](auto jj) {  // phase 1's reflectors
      constexpr int j = decltype(jj)::value, J1 = j + 1;
      const double *pj = sm.pv[q][j];
      const double scal = pj[0], tau = sm.tau[q][j];
      double u2a;
      if constexpr (J1 < J0) u2a = rbcast<J1>(uxP);
      else u2a = rbcast<0>(ux[0]);
      const double xP = (pre && l > J1) ? pj[lp] : 0.0;
      double x[NS], xu = xP * uxP;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        x[r] = pj[J0 + l + 16 * r];
        xu = fma(x[r], ux[r], xu);
      });
      xu = rsum16(xu);
      const double xsP = xP * scal;
      const double vP = (pre && l == J1) ? 1.0 : xsP;
      const double s2 = fma(scal, xu, u2a);  // v . x'
      uxP = fma(-tau * s2, vP, uxP);
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const double xs = x[r] * scal;
        double vr;
        if constexpr (J1 == J0 && r == 0) vr = l == 0 ? 1.0 : xs;
        else vr = xs;
        ux[r] = fma(-tau * s2, vr, ux[r]);
      });
    });
    sfor<KT - 2>([&](auto jj) {  // phase 2's reflectors
      constexpr int jl = decltype(jj)::value, j = J0 + jl;
      constexpr int J1 = jl + 1, R1 = J1 / 16, L1 = J1 % 16;
      const double scal = rbcast<L1>(A[R1][j]), tau = sm.tau[q][j];
      double x[NS], xu = 0.0;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 > J1) {
          const int t = l + 16 * r;
          if constexpr (r == R1) x[r] = t == J1 ? 0.0 : A[r][j];
          else x[r] = A[r][j];
          xu = fma(x[r], ux[r], xu);
        } else {
          x[r] = 0.0;
        }
      });
      xu = rsum16(xu);
      const double s2 = fma(scal, xu, rbcast<L1>(ux[R1]));  // v . x'
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int t = l + 16 * r;
        const double xs = x[r] * scal;
        const double vr = t == J1 ? 1.0 : xs;
        ux[r] = fma(-tau * s2, vr, ux[r]);
      });
    });
    if (pre) sm.tq[q][l][3] = uxP;
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      sm.tq[q][J0 + l + 16 * r][3] = ux[r];
    });
    __syncthreads();

    // ---- T^-1/2 u2 by quadrature, T^-1 u2 exactly (twin: solve_tq40_kernel's round loop) ---
    double ys[NV], z[NV];
    sfor<NV>([&](auto vv) { ys[decltype(vv)::value] = 0.0; });
    for (int round = 0; round < R; ++round) {
      const int node = 8 * round + n8;
      const double2 tw = qtab[min(node, NQ - 1)];
      const double sigma = node < NQ ? m * tw.x : 0.0;
      const double omega = node < NQ ? sqrt(m) * tw.y : 1.0;
      double hh[H], mm[H];
      unsigned pw = tq0;
      double dl = lds(pw) + sigma, gt = lds(pw + 24);
      double rdl = rcp64(dl);
      sfor<H - 1>([&](auto tt) {
        constexpr int t = decltype(tt)::value + 1;
        pw += dirb;
        asm volatile("" : "+v"(pw) : "v"(dl));  // row t is read once d_{t-1} is known
        const double ct = lds(pw + csb);
        const double lt = ct * rdl;
        hh[t - 1] = gt * rdl;
        mm[t - 1] = lt;
        dl = fma(-lt, ct, lds(pw) + sigma);
        gt = fma(-lt, gt, lds(pw + 24));
        rdl = rcp64(dl);
      });
      // rows H-1 (top) and H (bottom): 2x2 solve with the partner lane's pivot
      const double cm = T[H][1];
      const double dlo = ror8(dl), go = ror8(gt);
      double xv = (gt * dlo - cm * go) / fma(dl, dlo, -cm * cm);
      const bool last = round == R - 1;
      const bool zlane = last && n8 == 7;  // T^-1 u2: not a node of the sum
      const double om = zlane ? 0.0 : omega;
      unsigned ps = qs0;                          // qs of the walk's current row
      unsigned pz = qz0 + (zlane ? qs0 - (unsigned)offsetof(SM, qs) - (unsigned)q * KP * 8u
                                 : KP * 8u);     // qz of that row, or the dump word
      const unsigned zdir = zlane ? bdir : 0u;
      auto emit = [&](double x) {
        double s = om * x;
        s += dpp_f64<0xB1>(s);   // quad_perm [1,0,3,2]
        s += dpp_f64<0x4E>(s);   // quad_perm [2,3,0,1]
        s += dpp_f64<0x141>(s);  // row_half_mirror: the 8 lanes of the side
        // stores without branches: the side's 8 lanes store the same sum
        sts(ps, s);
        sts(pz, x);
      };
      emit(xv);
      sfor<H - 1>([&](auto tt) {
        constexpr int t = H - 2 - decltype(tt)::value;
        xv = fma(-mm[t], xv, hh[t]);
        ps += bdir;
        pz += zdir;
        asm volatile("" : "+v"(ps), "+v"(pz) : "v"(xv));
        emit(xv);
      });
      __syncthreads();
      sfor<NV>([&](auto vv) {
        constexpr int vs = decltype(vv)::value;
        const int i = vrow(vs);
        const int ic = i < KP ? i : 0;
        ys[vs] += i < KP ? sm.qs[q][ic] : 0.0;
        if (last) z[vs] = i < KP ? sm.qz[q][ic] : 0.0;
      });
      __syncthreads();
    }
    double dpart = 0.0;  // u1 . T^-1 u2 = wbar . x'
    sfor<NV>([&](auto vv) {
      constexpr int vs = decltype(vv)::value;
      const int i = vrow(vs);
      const double u1 = vs == 0 ? ubP : ub[vs > 0 ? vs - 1 : 0];
      dpart = i < KP ? fma(u1, z[vs], dpart) : dpart;
    });
    const double d = rsum16(dpart);

    // ---- back-transform: y <- Q y = H_0 H_1 ... H_{KP-3} y --------------------------------
    double y[NV];
    sfor<NV>([&](auto vv) { y[decltype(vv)::value] = ys[decltype(vv)::value]; });
    touch_cols();
    // (the lane index, redefined: the reflectors' unit rows, 1.0 where l == j + 1, are
    // selects of the lane index alone and would be kept across the loop, one per step)
    const int lb = touched(l);
    sfor<KT - 2>([&](auto jj) {  // phase 2's reflectors (rows > J0 only)
      constexpr int jl = KT - 3 - decltype(jj)::value, j = J0 + jl, J1 = jl + 1;
      constexpr int R1 = J1 / 16, L1 = J1 % 16;
      const double tj = sm.tau[q][j];
      const double scal = rbcast<L1>(A[R1][j]);
      double vv[NS], a = 0.0;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 >= J1) {
          const int t = lb + 16 * r;
          // column j's registers hold x, which is 0 on the rows < j + 1 (scal at row j + 1),
          // in the slots that step j wrote: the reflector is 1 at row j + 1 and x scal below
          if constexpr (16 * r + 15 > J1) vv[r] = t == J1 ? 1.0 : A[r][j] * scal;
          else vv[r] = t == J1 ? 1.0 : 0.0;
          a = fma(vv[r], y[r + 1], a);
        } else {
          vv[r] = 0.0;
        }
      });
      a = rsum16(a);
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 >= J1) y[r + 1] = fma(-tj * a, vv[r], y[r + 1]);
      });
    });
    sfor<J0>([&](auto jj) {  // phase 1's reflectors: pv's column j
      constexpr int j = J0 - 1 - decltype(jj)::value, J1 = j + 1;
      const double tj = sm.tau[q][j];
      const double *pj = sm.pv[q][j];
      const double scal = pj[0];
      const double v0 = lb == J1 ? 1.0 : (lb < J0 && lb > J1) ? pj[lb] * scal : 0.0;  // 0 at rows <= j + 1
      double vv[NS];
      double a = v0 * y[0];
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const double pr = pj[J0 + lb + 16 * r] * scal;
        if constexpr (J1 == J0 && r == 0) vv[r] = lb == 0 ? 1.0 : pr;
        else vv[r] = pr;
        a = fma(vv[r], y[r + 1], a);
      });
      a = rsum16(a);
      y[0] = fma(-tj * a, v0, y[0]);
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        y[r + 1] = fma(-tj * a, vv[r], y[r + 1]);
      });
    });

    // ---- analysis and RTPP / RTPS (:675-698), fp32 in the reference's order --------------
    // (twin: solve_tq40_kernel's epilogue, whose flags and alphas come from SolveConsts)
    float xa[NV];
    sfor<NV>([&](auto vv) {
      constexpr int vs = decltype(vv)::value;
      xa[vs] = vrow(vs) < k ? (float)(xb_mean + (d + sk * y[vs])) : 0.0f;
    });
    if (use_rtpp || use_rtps) {
      const float xa_mean = seq_sum_f32<KP>(xa) * c.nmember_inv;
      double xpl[NV];
      float xap[NV];
      sfor<NV>([&](auto vv) {
        constexpr int vs = decltype(vv)::value;
        const bool mem = vrow(vs) < k;
        xpl[vs] = mem ? (double)xbl[vs] - xb_mean : 0.0;
        xap[vs] = 0.0f;
        if (mem) {
          xap[vs] = xa[vs] - xa_mean;
          if (use_rtpp)
            xap[vs] = (float)((double)((1.0f - rtpp_alpha) * xap[vs]) +
                              (double)rtpp_alpha * xpl[vs]);
        }
      });
      if (use_rtps) {
        double d8 = 0.0;
        sfor<KP>([&](auto mm) {
          constexpr int mb = decltype(mm)::value;
          constexpr int vs = mb < J0 ? 0 : 1 + (mb - J0) / 16, ln = mb < J0 ? mb : (mb - J0) % 16;
          const double xp = rbcast<ln>(xpl[vs]);  // 0 past member k-1
          d8 = d8 + xp * xp;
        });
        const float xb_std = (float)d8;
        float sq[NV];
        sfor<NV>([&](auto vv) {
          constexpr int vs = decltype(vv)::value;
          sq[vs] = xap[vs] * xap[vs];
        });
        const float xa_std = seq_sum_f32<KP>(sq);
        const float f = rtps_alpha * sqrtf(xb_std / xa_std) - rtps_alpha + 1.0f;
        sfor<NV>([&](auto vv) { xap[decltype(vv)::value] = xap[decltype(vv)::value] * f; });
      }
      sfor<NV>([&](auto vv) { xa[decltype(vv)::value] = xa_mean + xap[decltype(vv)::value]; });
    }
    if (valid && ptot > 0) {
      const long long Ps = touched(P);
      sfor<NV>([&](auto vv) {
        constexpr int vs = decltype(vv)::value;
        const int i = vrow(vs);
        if (i < k) var[Ps + slab.L * touched(i)] = xa[vs];
      });
    }
  }
  // info.y: decade of the quadrature rule (negative when M/m exceeds the last table); once per
  // point (a wave that does not write reads info.x only, which keeps its value)
  if (valid && ptot > 0 && l == 0 && passes.writes_info())
    info[touched(gi)] = make_int2(ptot, ratio > dec ? -level : level);
}

}  // namespace cwbl
