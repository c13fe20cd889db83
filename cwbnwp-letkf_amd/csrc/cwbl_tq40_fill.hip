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
//                                 6880 + 640 B per point.
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
#include "cwbl_tq40_common.h"

#include <utility>

namespace cwbl {

namespace {

// Two row sums (the fill's steps' x.x and x.b1: rsum16x3 without the x' sum)
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

// The background gathers of a point, as loaded: member i = row i.  Branch-free, every address
// valid: a lane past the batch reads member 0 of point 0, a row past k member 0 of its point
// (tq40_factor_solve masks both to 0).  The hit issues these inside the factor's stream, so
// that the two HBM latencies overlap; the fill, whose registers are full until its factor is
// stored, just before the solve.
template <int KP>
__device__ __forceinline__ void tq40_load_xb(const SlabDev &slab, const long long g0,
                                             const bool valid, const int gi, const int l,
                                             const int k, float (&xv)[Tq40Layout<KP>::NV]) {
  const float *__restrict__ const var = slab.var;
  const long long P = tq40_var_index(slab, g0, valid ? gi : 0);  // var index of member 0
  sfor<Tq40Layout<KP>::NV>([&](auto vv) {
    constexpr int vs = decltype(vv)::value;
    const int i = tq40_vrow<KP>(l, vs);
    xv[vs] = var[P + slab.L * ((valid && i < k) ? i : 0)];
  });
}

// The call's variable from a point's factor.  On entry (after a barrier): sm.tq[q][i][0..2]
// hold d_i, c(i-1, i) and (Q^T b1)_i, sm.tau the steps' tau, sm.pv[q][j] phase 1's x with the
// step's scal in word 0, A[r][j] (j >= J0) phase 2's x with the step's scal at row j + 1.
// (Twin: solve_tq40_multi_kernel's variable loop body, with the flags
// and alphas of SolveConsts and slab.var.)
// AHEAD (the hit) changes the order of loads only, never an expression: the first round's
// node is fetched before the replay and each later one a round ahead, and the walk reads row
// t + 1 before d_{t-1}'s reciprocal.  That costs six VGPRs, which the fill does not have.
template <int KP, bool AHEAD>
__device__ __forceinline__ void tq40_factor_solve(
    const SolveConsts &c, const SlabDev &slab, Tq40Smem<KP> &sm,
    double (&A)[Tq40Layout<KP>::NS][KP], const float (&xbv)[Tq40Layout<KP>::NV], const long long g0,
    const bool valid, const int ptot, const int gi, const int q, const int l,
    int2 *__restrict__ info) {
  using LY = Tq40Layout<KP>;
  constexpr int J0 = LY::J0, KT = LY::KT, NS = LY::NS, NV = LY::NV, H = LY::H;
  using SM = Tq40Smem<KP>;
  const int k = c.k;
  const int lp = l < J0 ? l : 0;
  const bool pre = l < J0;
  auto vrow = [&](int vs) { return tq40_vrow<KP>(l, vs); };
  // the point's accepted count waits in LDS for the store at the end (row KP's word 3 is
  // unused; every lane of the row holds the same count): one register less across the solve
  int *const pkeep = reinterpret_cast<int *>(&sm.tq[q][KP][3]);
  *pkeep = ptot;
  const double trace = tq40_trace(sm, q, l, k);

  // ---- the quadrature rule of the point: T only ---------------------------------------------
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
  double2 twn;  // AHEAD: the next round's node, in flight
  if constexpr (AHEAD) twn = qtab[min(l & 7, NQ - 1)];
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
  // back-transform derive from them (x scal, the scal broadcasts, the row j + 1 selects) would
  // otherwise be shared across the quadrature and double the live registers
  auto touch_cols = [&]() {
    sfor<KT - 2>([&](auto jj) {
      constexpr int jl = decltype(jj)::value, J1 = jl + 1, R1 = J1 / 16;
      sfor<NS>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        if constexpr (16 * r + 15 > J1 || r == R1) touch(A[r][J0 + jl]);
      });
    });
  };

  float *__restrict__ const var = slab.var;
  const int use_rtpp = c.use_rtpp, use_rtps = c.use_rtps;
  const float rtpp_alpha = c.rtpp_alpha, rtps_alpha = c.rtps_alpha;

  // background of the point: member i = row i (xbv: tq40_load_xb's gathers)
  float xbl[NV];
  double xb_mean;
  {
    sfor<NV>([&](auto vv) {
      constexpr int vs = decltype(vv)::value;
      const bool mem = valid && vrow(vs) < k;
      xbl[vs] = mem ? xbv[vs] : 0.0f;
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

  // ---- replay: x' <- Q^T x', the x' half of every step of solve_tq40_kernel ----------------
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
    // (touch_cols, column by column: on a hit the column may still be in flight until here)
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      if constexpr (16 * r + 15 > J1 || r == R1) touch(A[r][j]);
    });
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

  // ---- T^-1/2 u2 by quadrature, T^-1 u2 exactly (twin: solve_tq40_kernel's round loop) -----
  double ys[NV], z[NV];
  sfor<NV>([&](auto vv) { ys[decltype(vv)::value] = 0.0; });
  for (int round = 0; round < R; ++round) {
    const int node = 8 * round + n8;
    double2 tw;
    if constexpr (AHEAD) {
      tw = twn;
      // the next round's node, one round ahead (R is wave-uniform: no divergence)
      if (round + 1 < R) twn = qtab[min(node + 8, NQ - 1)];
    } else {
      tw = qtab[min(node, NQ - 1)];
    }
    const double sigma = node < NQ ? m * tw.x : 0.0;
    const double omega = node < NQ ? sqrt(m) * tw.y : 1.0;
    double hh[H], mm[H];
    unsigned pw = tq0;
    double dl = lds(pw) + sigma, gt = lds(pw + 24);
    // The next row's three words, read once d_{t-1} is known (the empty asm: read earlier,
    // all H rows would be live at once).  AHEAD reads row t + 1 there, before d_{t-1}'s
    // reciprocal, so that the LDS round trip runs under the rcp64 chain (rows 1 .. H-1 only:
    // never past the walk); otherwise it is row t, one register triple less.
    double nd, nc, ng;
    auto next_row = [&]() {
      pw += dirb;
      nd = lds(pw);
      nc = lds(pw + csb);
      ng = lds(pw + 24);
    };
    if constexpr (AHEAD) next_row();
    sfor<H - 1>([&](auto tt) {
      constexpr int t = decltype(tt)::value + 1;
      if constexpr (!AHEAD) {
        asm volatile("" : "+v"(pw) : "v"(dl));
        next_row();
      }
      const double dt = nd, ct = nc, g = ng;
      if constexpr (AHEAD && t < H - 1) {
        asm volatile("" : "+v"(pw) : "v"(dl));
        next_row();
      }
      const double rdl = rcp64(dl);
      const double lt = ct * rdl;
      hh[t - 1] = gt * rdl;
      mm[t - 1] = lt;
      dl = fma(-lt, ct, dt + sigma);
      gt = fma(-lt, gt, g);
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
    // ((Q^T b1)_i from LDS: kept in registers it would be live across the quadrature)
    const double u1 = sm.tq[q][i < KP ? i : 0][2];
    dpart = i < KP ? fma(u1, z[vs], dpart) : dpart;
  });
  const double d = rsum16(dpart);

  // ---- back-transform: y <- Q y = H_0 H_1 ... H_{KP-3} y ------------------------------------
  double y[NV];
  sfor<NV>([&](auto vv) { y[decltype(vv)::value] = ys[decltype(vv)::value]; });
  touch_cols();
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

  // ---- analysis and RTPP / RTPS (:675-698), fp32 in the reference's order ------------------
  // (twin: solve_tq40_kernel's epilogue)
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
      // sum of xp^2 in member order: the squares per lane (the products of the broadcast
      // values, formed once), then one fused row add each (x 1.0: the add's one rounding)
      double d8 = 0.0, sq8[NV];
      sfor<NV>([&](auto vv) {
        constexpr int vs = decltype(vv)::value;
        sq8[vs] = xpl[vs] * xpl[vs];  // 0 past member k-1
        dpp_pin(sq8[vs]);
      });
      sfor<KP>([&](auto mm) {
        constexpr int mb = decltype(mm)::value;
        constexpr int vs = mb < J0 ? 0 : 1 + (mb - J0) / 16, ln = mb < J0 ? mb : (mb - J0) % 16;
        d8 = fmac_row<ln>(d8, sq8[vs], 1.0);
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
  const int pt = *pkeep;
  if (valid && pt > 0) {
    // (the point's var index again, from gi redefined: kept from the loads on, it would hold
    // two registers across the whole solve)
    const long long P = tq40_var_index(slab, g0, touched(gi));
    sfor<NV>([&](auto vv) {
      constexpr int vs = decltype(vv)::value;
      const int i = vrow(vs);
      if (i < k) var[P + slab.L * i] = xa[vs];
    });
    // info.y: decade of the quadrature rule (negative when M/m exceeds the last table)
    if (l == 0) info[gi] = make_int2(pt, ratio > dec ? -level : level);
  }
}

}  // namespace

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

// ---- the hit: the call's variable from the kept factor -----------------------------------------
template <int KP>
__global__ void __launch_bounds__(64, 2)
solve_tq40_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                         const double *__restrict__ ws, const double *__restrict__ aux,
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
  const int ptot = valid ? info[gi].x : 0;
  const bool pre = l < J0;

  // ---- the factor's loads: the wave's four factors through a buffer resource, as
  // tq40_load_record reads records (a lane past the batch reads the spare one, npts).  Lane l
  // of a row reads word l of each 16-row run of a column: 128 contiguous bytes per row.
  const __amdgpu_buffer_rsrc_t rs = rec_rsrc(ws + (size_t)(4 * g4) * FR::WORDS, 4 * FR::WORDS);
  const unsigned rq = (unsigned)(valid ? q : npts - 4 * g4) * (unsigned)FR::WORDS;
  // factor word vword + cword (cword static: the low 12 bits of its byte offset fold into the
  // instruction's offset field, the rest is one of two scalar offsets)
  auto rw = [&](unsigned vword, unsigned cword) {
    const unsigned cb = 8u * cword;
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(8u * vword + (cb & 4095u)),
                                                        (int)(cb & ~4095u), 0);
    return __longlong_as_double(((long long)v[1] << 32) | (unsigned)v[0]);
  };
  // the same from a byte offset, which may be kRecSkip: that lane loads 0 without an access
  auto rwb = [&](unsigned vbyte, unsigned cword) {
    const unsigned cb = 8u * cword;
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(vbyte + (cb & 4095u)),
                                                        (int)(cb & ~4095u), 0);
    return __longlong_as_double(((long long)v[1] << 32) | (unsigned)v[0]);
  };
  const unsigned rl = rq + (unsigned)l;
  // Loads return in order, so they go out in the order of their first use: T, Q^T b1 and the
  // steps' scalars (the trace, the level and every replay step need them), then phase 1's
  // columns, then phase 2's, which the replay's first J0 steps leave in flight.
  double dg[(KP + 15) / 16];
  sfor<(KP + 15) / 16>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int i = l + 16 * r;
    dg[r] = rw(rq + (unsigned)(i < KP ? i : 0), (unsigned)FR::D);
  });
  double ubP, ub[NS];
  {
    const double b = rw(rq + (unsigned)(pre ? l : 0), (unsigned)FR::U1);
    ubP = pre ? b : 0.0;
  }
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    ub[r] = rw(rl, (unsigned)(FR::U1 + J0 + 16 * r));
  });
  // the steps' beta and tau: the wave's four FactorAux entries, the same way (the spare entry
  // for a lane past the batch).  Lane l takes words l, l + 16 and, l < 8, l + 32 of each half;
  // the lanes >= 8 take word l + 16 again, and store it again below.
  const __amdgpu_buffer_rsrc_t ra = rec_rsrc(aux + (size_t)(4 * g4) * FA::WORDS, 4 * FA::WORDS);
  const unsigned aq = (unsigned)(valid ? q : npts - 4 * g4) * (unsigned)FA::WORDS;
  constexpr int NA = (KP + 15) / 16;
  static_assert(16 * (NA - 1) + 8 == KP, "the last run of an aux half is half a row");
  const int l2 = l < 8 ? l + 16 * (NA - 1) : l + 16 * (NA - 2);
  auto arow = [&](int r) { return r < NA - 1 ? l + 16 * r : l2; };
  double bt[NA], ta[NA];
  sfor<NA>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const unsigned off = 8u * (aq + (unsigned)arow(r));
    const auto vb = __builtin_amdgcn_raw_buffer_load_b64(ra, (int)(off + 8u * FA::B), 0, 0);
    const auto vt = __builtin_amdgcn_raw_buffer_load_b64(ra, (int)(off + 8u * FA::T), 0, 0);
    bt[r] = __longlong_as_double(((long long)vb[1] << 32) | (unsigned)vb[0]);
    ta[r] = __longlong_as_double(((long long)vt[1] << 32) | (unsigned)vt[0]);
  });
  double A[NS][KP];     // phase 2's columns J0 .. KP-3 only: scal at row j + 1, x below, 0 above
  // phase 1's columns: c1P is x on the prefix rows > j + 1 and the step's scal (the column's
  // first word, row j + 1) on every other lane
  double c1P[J0], c1[J0][NS];
  sfor<J0>([&](auto jj) {
    constexpr int j = decltype(jj)::value, J1 = j + 1;
    c1P[j] = rw(rq + (unsigned)((pre && l > J1) ? l - J1 : 0), (unsigned)FR::col(j));
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      // (step J0-1: row j + 1 = J0 is lane 0 of slot 0, whose x is 0)
      if constexpr (J1 == J0 && r == 0)
        c1[j][r] = rwb(rec_off(l != 0, (int)rl), (unsigned)(FR::col(j) + J0 + 16 * r - J1));
      else
        c1[j][r] = rw(rl, (unsigned)(FR::col(j) + J0 + 16 * r - J1));
    });
  });
  // The background gathers ride in the same stream, so the wave pays one HBM latency, not two:
  // behind everything the solve needs before them (their address arithmetic would hold the
  // stream's first load back by a hundred instructions) and ahead of phase 2's columns.
  float xv[LY::NV];
  tq40_load_xb<KP>(slab, g0, valid, gi, l, c.k, xv);
  sfor<KT - 2>([&](auto jj) {
    constexpr int jl = decltype(jj)::value, j = J0 + jl, J1 = jl + 1;
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      if constexpr (16 * r >= J1) {
        A[r][j] = rw(rl, (unsigned)(FR::col(j) + 16 * r - J1));
      } else if constexpr (16 * r + 15 >= J1) {  // the rows above j + 1 are 0
        const int t = l + 16 * r;
        A[r][j] = rwb(rec_off(t >= J1, (int)rq + t - J1), (unsigned)FR::col(j));
      }
    });
  });

  // ---- T's diagonal and off-diagonal, Q^T b1 and the steps' tau ---------------------------------
  sfor<(KP + 15) / 16>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int i = l + 16 * r;
    sm.tq[q][i < KP ? i : KP][0] = dg[r];  // (row KP's words 0, 2, 3 are unused: the dump)
  });
  sm.tq[q][pre ? l : KP][2] = ubP;
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    sm.tq[q][J0 + l + 16 * r][2] = ub[r];
  });
  // T's off-diagonal (word 0 is 0, word KP-1 the trailing 2 x 2's) and tau as the fill's steps
  // left them in LDS; row KP's off-diagonal closes the walk from the bottom
  sfor<NA>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    sm.tq[q][arow(r)][1] = bt[r];
    sm.tau[q][arow(r)] = ta[r];
  });
  sm.tq[q][KP][1] = 0.0;  // (every lane of the row stores the same value: no branch)

  // ---- the reflectors, where solve_tq40_multi_kernel keeps them -----------------------------------
  // phase 1: sm.pv[q][j] holds x by row and the step's scal in word 0, which the lanes without
  // a prefix row of x store (the same value from each); phase 2's columns are in place as
  // loaded
  sfor<J0>([&](auto jj) {
    constexpr int j = decltype(jj)::value, J1 = j + 1;
    sm.pv[q][j][(pre && l > J1) ? l : 0] = c1P[j];
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      sm.pv[q][j][J0 + l + 16 * r] = c1[j][r];
    });
  });
  __syncthreads();

  tq40_factor_solve<KP, true>(c, slab, sm, A, xv, g0, valid, ptot, gi, q, l, info);
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
