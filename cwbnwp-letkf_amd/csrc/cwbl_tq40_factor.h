// cwbl_tq40_factor.h — what the kernels of the cached factor share (cwbl_tq40_fill.hip: the fill
// and the hit of one batch; cwbl_tq40_hit_merge.hip: the hit of several): the solve of the
// call's variable from a point's factor, and the hit's block, which loads the factor first.
#pragma once

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

// LEAN: sm.tq's rows, sm.qs and sm.qz stand in the order the twisted walk takes them: side 0's
// rows 0 .. H-1, then side 1's rows KP-1 .. H, so that both sides step through them with the
// same compile-time stride.  Word 1 of a slot is the coupling with the walk's row before it
// (side 0: c(i-1, i); side 1: c(i, i+1)); the middle coupling c(H-1, H) is word 1 of row KP.
template <int KP>
__device__ __forceinline__ int tq40_walk_slot(int i) {
  constexpr int H = KP / 2;
  return i < H ? i : KP + H - 1 - i;
}
// the same for a row of the 16 from LO on (i < KP), and the row itself without LEAN
template <int KP, bool LEAN, int LO>
__device__ __forceinline__ int tq40_slot16(int i) {
  constexpr int H = KP / 2;
  if constexpr (!LEAN || LO + 15 < H) return i;
  else if constexpr (LO >= H) return KP + H - 1 - i;
  else return tq40_walk_slot<KP>(i);
}
// where T's off-diagonal word i = c(i-1, i) goes (word 0, which is 0, and the coupling of a
// side's first row are never read)
template <int KP>
__device__ __forceinline__ int tq40_walk_cslot(int i) {
  constexpr int H = KP / 2;
  return i < H ? i : i == H ? KP : KP + H - i;
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
// LEAN (the merged hit alone) changes where a value is kept and which lanes a select masks,
// never an expression either: the replay leaves each step's reflector v (1 at row j + 1,
// x scal below) where it found x (phase 1: sm.pv's column, phase 2: the column's registers),
// and the back-transform takes it from there instead of forming the same product again; phase
// 2's columns may hold any words on the rows above j + 1 (tq40_factor_hit's plain loads).
// It also takes a solved point's level from ly, the info.y its fill stored, instead of
// working it out again from the trace (cuts: HitLevelCuts of the call's inflat and k, for the
// lanes that have no kept level; see there; profiles/hit_masks.txt).
template <int KP, bool AHEAD, bool LEAN = false>
__device__ __forceinline__ void tq40_factor_solve(
    const SolveConsts &c, const SlabDev &slab, Tq40Smem<KP> &sm,
    double (&A)[Tq40Layout<KP>::NS][KP], const float (&xbv)[Tq40Layout<KP>::NV], const long long g0,
    const bool valid, const int ptot, const int gi, const int q, const int l,
    int2 *__restrict__ info, const int ly = 0, const HitLevelCuts &cuts = HitLevelCuts{}) {
  using LY = Tq40Layout<KP>;
  constexpr int J0 = LY::J0, KT = LY::KT, NS = LY::NS, NV = LY::NV, H = LY::H;
  using SM = Tq40Smem<KP>;
  const int k = c.k;
  const int lp = l < J0 ? l : 0;
  const bool pre = l < J0;
  auto vrow = [&](int vs) { return tq40_vrow<KP>(l, vs); };
  // slot of sm.tq, sm.qs and sm.qz of row i = vrow(vs), 0 where the lane has no such row
  // (the row itself without LEAN)
  auto vslot = [&](auto vv, int i) {
    constexpr int vs = decltype(vv)::value;
    if constexpr (!LEAN || vs == 0) return i < KP ? i : 0;  // (J0 <= H)
    else return tq40_slot16<KP, true, J0 + 16 * (vs > 0 ? vs - 1 : 0)>(i);
  };
  static_assert(J0 <= H, "the prefix rows are side 0's");
  // the point's accepted count waits in LDS for the store at the end (row KP's word 3 is
  // unused; every lane of the row holds the same count): one register less across the solve
  int *const pkeep = reinterpret_cast<int *>(&sm.tq[q][KP][3]);
  *pkeep = ptot;
  if constexpr (LEAN) pkeep[1] = ly;  // (and the kept info.y beside it)

  // ---- the quadrature rule of the point: T only ---------------------------------------------
  // (twin: this level loop and the walk's LDS offsets below are solve_tq40_kernel's)
  const double m = (double)c.inflat;
  int level = 1;
  double ratio = 0.0, dec = 10.0;
  if constexpr (LEAN) {
    // The level is a function of the factor and of inflat, which the cache's key holds, and the
    // fill's solve has stored it: ly = info.y is +-level on a point with p > 0, as this text
    // left it there on the fill (negative: M/m beyond the last table), and what is stored at
    // the end is ly again.  ly = 0 marks the lanes no solve has written for: a point with
    // p = 0, whose info the assembly left as (0, 0), and a lane past the segment.  Their
    // records are whatever the cache's memory held (the assembly skips a point with p = 0, the
    // spare record is never written), so no constant stands for their level; but it reaches
    // nothing of a stored result except the wave's rounds R, through quad_rounds, which steps
    // after the levels kRoundCuts alone.  The loop below ends above level n < kQuadLevels
    // exactly when 10^n < trace / m - (k - 1) (the decades are exact, and each test implies
    // the one before it).  For m >= 0 the rounded quotient and the rounded difference do not
    // decrease with the trace, so that holds from a smallest trace on, cuts.t, which the host
    // finds by bisection with the same two operations; a NaN trace fails the test and the
    // compare alike.  Such a lane takes the first level of its class of rounds, and its own
    // rule, sums and analysis, which are never stored, may differ from the loop's.  Only a
    // wave that has such a lane sums its traces (wave-uniform: no lane is masked off).
    const bool known = ly != 0;
    level = min(max(abs(ly), 1), kQuadLevels);
    if (__ballot(!known)) {
      double tp = 0.0;  // tq40_trace through the slots
      sfor<(KP + 15) / 16>([&](auto rr) {
        constexpr int r = decltype(rr)::value;
        const int i = l + 16 * r;
        if (16 * r + 15 < KP || i < KP)
          tp += i < k ? sm.tq[q][i < KP ? tq40_slot16<KP, true, 16 * r>(i) : 0][0] : 0.0;
      });
      const double trace = rsum16(tp);
      const int lt = trace >= cuts.t[2]   ? kRoundCuts[2] + 1
                     : trace >= cuts.t[1] ? kRoundCuts[1] + 1
                     : trace >= cuts.t[0] ? kRoundCuts[0] + 1
                                          : 1;
      level = known ? level : lt;
    }
  } else {
    const double trace = tq40_trace(sm, q, l, k);
    ratio = trace / m - (double)(k - 1);
    while (level < kQuadLevels && dec < ratio) {
      dec *= 10.0;
      ++level;
    }
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
                       (LEAN ? (side ? H * 32u : 0u)
                             : (side ? (KP - 1) * 32u : 0u));   // row 0 of the walk
  const unsigned dirb = side ? (unsigned)-32 : 32u;   // next row of the walk
  const unsigned csb = side ? 40u : 8u;  // coupling with the previous row of the walk
  const unsigned qs0 = (unsigned)(offsetof(SM, qs) + (size_t)q * sizeof(sm.qs[0])) +
                       (LEAN ? (side ? H * 8u : 0u)            // LEAN: row 0 of the walk
                             : (side ? (KP - H) * 8u : (H - 1) * 8u));  // row H-1 of the walk
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
    double *const pj = sm.pv[q][j];
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
      if constexpr (LEAN) pj[J0 + l + 16 * r] = vr;
    });
    // LEAN: v over x, row by row; the lanes without a prefix row store into word 0, the scal
    // this step has read, and the prefix rows <= j + 1 into their own unused words
    if constexpr (LEAN) pj[lp] = vP;
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
        if constexpr (r == R1 && LEAN) x[r] = t > J1 ? A[r][j] : 0.0;
        else if constexpr (r == R1) x[r] = t == J1 ? 0.0 : A[r][j];
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
      if constexpr (LEAN && 16 * r + 15 > J1) A[r][j] = vr;
    });
  });
  if (pre) sm.tq[q][l][3] = uxP;
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    sm.tq[q][tq40_slot16<KP, LEAN, J0 + 16 * r>(J0 + l + 16 * r)][3] = ux[r];
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
    auto next_row = [&](auto ww) {
      if constexpr (LEAN) {  // walk row ww: the slots are in walk order, the base stays
        constexpr unsigned wo = 32u * (unsigned)decltype(ww)::value;
        nd = lds(pw + wo);
        nc = lds(pw + wo + 8);
        ng = lds(pw + wo + 24);
      } else {
        pw += dirb;
        nd = lds(pw);
        nc = lds(pw + csb);
        ng = lds(pw + 24);
      }
    };
    if constexpr (AHEAD) next_row(std::integral_constant<int, 1>{});
    sfor<H - 1>([&](auto tt) {
      constexpr int t = decltype(tt)::value + 1;
      if constexpr (!AHEAD) {
        asm volatile("" : "+v"(pw) : "v"(dl));
        next_row(std::integral_constant<int, t>{});
      }
      const double dt = nd, ct = nc, g = ng;
      if constexpr (AHEAD && t < H - 1) {
        asm volatile("" : "+v"(pw) : "v"(dl));
        next_row(std::integral_constant<int, t + 1>{});
      }
      const double rdl = rcp64(dl);
      const double lt = ct * rdl;
      hh[t - 1] = gt * rdl;
      mm[t - 1] = lt;
      dl = fma(-lt, ct, dt + sigma);
      gt = fma(-lt, gt, g);
    });
    // rows H-1 (top) and H (bottom): 2x2 solve with the partner lane's pivot
    const double cm = T[LEAN ? KP : H][1];
    const double dlo = ror8(dl), go = ror8(gt);
    double xv = (gt * dlo - cm * go) / fma(dl, dlo, -cm * cm);
    const bool last = round == R - 1;
    const bool zlane = last && n8 == 7;  // T^-1 u2: not a node of the sum
    const double om = zlane ? 0.0 : omega;
    unsigned ps = qs0;                          // qs of the walk's current row (LEAN: row 0)
    // qz of that row, or the dump word.  LEAN has no dump: a lane that is not the z lane puts
    // its x where the side's sum goes, and the sum's store, which follows, overwrites it
    unsigned pz = LEAN ? (zlane ? qz0 + (side ? H * 8u : 0u) : qs0)
                       : qz0 + (zlane ? qs0 - (unsigned)offsetof(SM, qs) - (unsigned)q * KP * 8u
                                      : KP * 8u);
    const unsigned zdir = zlane ? bdir : 0u;
    auto emit = [&](double x, auto ww) {
      double s = om * x;
      s += dpp_f64<0xB1>(s);   // quad_perm [1,0,3,2]
      s += dpp_f64<0x4E>(s);   // quad_perm [2,3,0,1]
      s += dpp_f64<0x141>(s);  // row_half_mirror: the 8 lanes of the side
      // stores without branches: the side's 8 lanes store the same sum
      if constexpr (LEAN) {
        constexpr unsigned wo = 8u * (unsigned)decltype(ww)::value;
        sts(pz + wo, x);
        sts(ps + wo, s);
      } else {
        sts(ps, s);
        sts(pz, x);
      }
    };
    emit(xv, std::integral_constant<int, H - 1>{});
    sfor<H - 1>([&](auto tt) {
      constexpr int t = H - 2 - decltype(tt)::value;
      xv = fma(-mm[t], xv, hh[t]);
      if constexpr (!LEAN) {
        ps += bdir;
        pz += zdir;
      }
      asm volatile("" : "+v"(ps), "+v"(pz) : "v"(xv));
      emit(xv, std::integral_constant<int, t>{});
    });
    __syncthreads();
    sfor<NV>([&](auto vv) {
      constexpr int vs = decltype(vv)::value;
      const int i = vrow(vs);
      const int ic = vslot(vv, i);
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
    const double u1 = sm.tq[q][vslot(vv, i)][2];
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
    double scal;
    if constexpr (!LEAN) scal = rbcast<L1>(A[R1][j]);
    double vv[NS], a = 0.0;
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      if constexpr (16 * r + 15 >= J1) {
        const int t = lb + 16 * r;
        // column j's registers hold x, which is 0 on the rows < j + 1 (scal at row j + 1),
        // in the slots that step j wrote: the reflector is 1 at row j + 1 and x scal below
        if constexpr (16 * r + 15 > J1) {
          if constexpr (LEAN) vv[r] = A[r][j];  // the replay's v
          else vv[r] = t == J1 ? 1.0 : A[r][j] * scal;
        } else {
          vv[r] = t == J1 ? 1.0 : 0.0;
        }
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
    double scal, v0;
    if constexpr (!LEAN) {
      scal = pj[0];
      v0 = lb == J1 ? 1.0 : (lb < J0 && lb > J1) ? pj[lb] * scal : 0.0;  // 0 at rows <= j + 1
    } else if constexpr (J1 == J0) {
      v0 = lb == J1 ? 1.0 : 0.0;
    } else {
      v0 = (lb < J0 && lb >= J1) ? pj[lb] : 0.0;  // the replay's v
    }
    double vv[NS];
    double a = v0 * y[0];
    sfor<NS>([&](auto rr) {
      constexpr int r = decltype(rr)::value;
      if constexpr (LEAN) {
        vv[r] = pj[J0 + lb + 16 * r];
      } else {
        const double pr = pj[J0 + lb + 16 * r] * scal;
        if constexpr (J1 == J0 && r == 0) vv[r] = lb == 0 ? 1.0 : pr;
        else vv[r] = pr;
      }
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
    // (LEAN: the kept word, which is that)
    if constexpr (LEAN) {
      if (l == 0) info[gi] = make_int2(pt, pkeep[1]);
    } else {
      if (l == 0) info[gi] = make_int2(pt, ratio > dec ? -level : level);
    }
  }
}

}  // namespace

// ---- the hit: the call's variable from the kept factor -----------------------------------------
// Block b of the nblk that cover the npts points from g0 (records ws, entries aux, info as of
// launch_solve_tq40_factor): the whole of solve_tq40_factor_kernel, and of a segment's block
// of solve_tq40_factor_merged_kernel.
// LEAN: the merged kernel's variant (tq40_factor_solve's, and plain loads of phase 2's columns).
template <int KP, bool LEAN = false>
__device__ __forceinline__ void tq40_factor_hit(const SolveConsts &c, const SlabDev &slab,
                                                const long long g0,
                                                const int npts, const double *__restrict__ ws,
                                                const double *__restrict__ aux,
                                                int2 *__restrict__ info, const int b,
                                                const int nblk,
                                                const HitLevelCuts &cuts = HitLevelCuts{}) {
  using LY = Tq40Layout<KP>;
  using FR = FactorRecord<KP>;
  using FA = FactorAux<KP>;
  constexpr int J0 = LY::J0, KT = LY::KT, NS = LY::NS;
  using SM = Tq40Smem<KP>;
  __shared__ SM sm;

  const int lane = threadIdx.x, q = lane >> 4, l = lane & 15;
  // the order of solve_tq40_kernel: XCD by XCD, each XCD's chunk from its end
  const int g4 = xcd_remap_rev(b, nblk);
  const int gi = 4 * g4 + q;
  const bool valid = gi < npts;
  int ptot, ly = 0;
  if constexpr (LEAN) {  // (p, +-level) as the fill's solve left them
    const int2 pi = valid ? info[gi] : make_int2(0, 0);
    ptot = pi.x;
    ly = pi.x > 0 ? pi.y : 0;
  } else {
    ptot = valid ? info[gi].x : 0;
  }
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
        // (LEAN: or words of the columns before, in the same record, which the replay masks)
        if constexpr (LEAN) A[r][j] = rw(rl, (unsigned)(FR::col(j) + 16 * r - J1));
        else A[r][j] = rwb(rec_off(t >= J1, (int)rq + t - J1), (unsigned)FR::col(j));
      }
    });
  });

  // ---- T's diagonal and off-diagonal, Q^T b1 and the steps' tau ---------------------------------
  sfor<(KP + 15) / 16>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int i = l + 16 * r;
    // (row KP's words 0, 2, 3 are unused: the dump)
    sm.tq[q][i < KP ? tq40_slot16<KP, LEAN, 16 * r>(i) : KP][0] = dg[r];
  });
  sm.tq[q][pre ? l : KP][2] = ubP;
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    sm.tq[q][tq40_slot16<KP, LEAN, J0 + 16 * r>(J0 + l + 16 * r)][2] = ub[r];
  });
  // T's off-diagonal (word 0 is 0, word KP-1 the trailing 2 x 2's) and tau as the fill's steps
  // left them in LDS; row KP's off-diagonal closes the walk from the bottom
  sfor<NA>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    sm.tq[q][LEAN ? tq40_walk_cslot<KP>(arow(r)) : arow(r)][1] = bt[r];
    sm.tau[q][arow(r)] = ta[r];
  });
  // (every lane of the row stores the same value: no branch; LEAN keeps c(H-1, H) there, and
  // the coupling above side 1's first row is never read)
  if constexpr (!LEAN) sm.tq[q][KP][1] = 0.0;

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

  tq40_factor_solve<KP, true, LEAN>(c, slab, sm, A, xv, g0, valid, ptot, gi, q, l, info, ly,
                                    cuts);
}

}  // namespace cwbl
