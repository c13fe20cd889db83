// cwbl_tq_big_factor.h — what the factor cache's kernel files of the hand-off path share
// (cwbl_tq_big_factor.hip: KP = 96, CWBL_OPT_BIG_REUSE; cwbl_tq_rows_factor.hip: KP = 128,
// CWBL_OPT_ROWS_REUSE): the point index, tqb_finish (the quadrature, back-transform and epilogue
// over two row loaders) and fill_tqb_tail_kernel<KP, J0>, the tail's text with the factor's
// stores.  Each file instantiates the fill at its own KP and has its own hit kernel.  As a
// header the text leaves the two <96, 32> kernels' instruction streams as they were
// (profiles/rows_reuse.txt).  tqb_factor_hit is the <96, 32> hit kernel's body as a function:
// solve_tqb_factor_kernel calls it once, the level kernel of a column-shared call
// (cwbl_tq_big_column.hip, CWBL_OPT_COLUMN_FACTOR) once per level; the hit kernel's assembly
// equals the parent's in every line (profiles/column_factor.txt).
#pragma once

#include "cwbl_tq_tail_common.h"

#include <utility>

namespace cwbl {

namespace {

// var index of member 0 of point g
__device__ __forceinline__ long long bf_point_index(const SlabDev &slab, long long g) {
  const int i = (int)(g % slab.ix_lim);
  const long long rr = g / slab.ix_lim;
  const int jj = (int)(rr % slab.iy_lim);
  const int kz = (int)(rr / slab.iy_lim);
  return i + (long long)slab.nx * (jj + (long long)slab.ny * kz);
}

// What follows the Householder loop in solve_tqb_tail_kernel, from the quadrature level to the
// stores: sm.tq, sm.tau and sm.scl are as the loop leaves them (behind a barrier).  Lane l
// holds rows l (slot 0, l < J0) and J0 + l (slot 1).  The reflector rows come through the
// loaders: ld_tail(jl, live) is the raw pivot row entry of row J0 + l of the tail's step jl
// (0 where !live), ld_hand(J, x0, x1) rows l and J0 + l of the hand-off kernel's reflector j
// (x0 zero at rows <= j).
// INFO (the default): info[gi] is stored; a level of a column-shared call stores none.
template <int KP, int J0, bool INFO = true, class LdTail, class LdHand>
__device__ __forceinline__ void tqb_finish(TailSmem<KP, J0> &sm, const SolveConsts &c,
                                           const SlabDev &slab, int gi, int l, int k, long long P,
                                           float xb0, float xb1, bool mem0, bool mem1,
                                           double trace, int ptot, int2 *__restrict__ info,
                                           LdTail ld_tail, LdHand ld_hand) {
  constexpr int KT = KP - J0;
  constexpr int H = KP / 2;
  const int nst = k - 2 - J0;
  // ---- T^-1/2 u2 by quadrature, u1^T T^-1 u2 exactly (solve_tq_big_kernel's rule) --------
  const double m = (double)c.inflat;
  const double ratio = trace / m - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }
  {
    const int node = l & 31, side = l >> 5;
    const int npass = quad_passes(level);
    const double2 *rule = quad_rule(c.quad_r, npass == 1 ? 4 : 8, level);
    for (int pass = 0; pass < npass; ++pass) {
    const bool exact = pass == 0 && node == 31;
    double sigma = 0.0, omega = 0.0;
    if (!exact) {
      const double2 tw = rule[31 * pass + node];
      sigma = m * tw.x;
      omega = sqrt(m) * tw.y;
    }
    // byte offsets into sm.tq: row t of the walk at q0 + dirb t (opaque_after, cwbl_device.h)
    const unsigned q0 = side ? (KP - 1) * 32u : 0u, dirb = side ? (unsigned)-32 : 32u;
    const unsigned csb = side ? 40u : 8u;  // coupling with the previous row of the walk
    auto fwd = [&](int t, double &dl, double &gt) {
      const unsigned o = opaque_after(q0, dl) + dirb * (unsigned)t;
      const double ct = lds_at(sm.tq, o + csb);
      const double lt = ct * rcp64(dl);
      dl = fma(-lt, ct, lds_at(sm.tq, o) + sigma);
      gt = fma(-lt, gt, lds_at(sm.tq, o + 24));
    };
    constexpr int S = 8, NS = H / S;
    double ckd[NS], ckg[NS];
    double dl = lds_at(sm.tq, q0) + sigma, gt = lds_at(sm.tq, q0 + 24);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      ckd[s] = dl;
      ckg[s] = gt;
#pragma unroll
      for (int t = S * s + 1; t < S * s + S; ++t) fwd(t, dl, gt);
      if (s + 1 < NS) fwd(S * s + S, dl, gt);
    }
    const double cm = sm.tq[H][1];  // meeting rows H-1 (top) and H (bottom)
    const double dlo = __shfl_xor(dl, 32, 64), go = __shfl_xor(gt, 32, 64);
    double xv = (gt * dlo - cm * go) / fma(dl, dlo, -cm * cm);
    double *ym = sm.Ym + side * H, *zm = sm.Zm + side * H;
    for (int s = NS - 1; s >= 0; --s) {
      double hh[S], mmv[S];
      double d2 = ckd[s], g2 = ckg[s];
#pragma unroll
      for (int i = 0; i < S; ++i) {
        const int t = S * s + i;
        if (i > 0) fwd(t, d2, g2);
        const double rd = rcp64(d2);
        hh[i] = g2 * rd;
        mmv[i] = (t + 1 < H)  // c_{t+1} / dl_t
                     ? lds_at(sm.tq, opaque_after(q0, d2) + dirb * (unsigned)(t + 1) + csb) * rd
                     : 0.0;
      }
#pragma unroll
      for (int i = S - 1; i >= 0; --i) {
        const int t = S * s + i;
        if (t != H - 1) xv = fma(-mmv[i], xv, hh[i]);
        const double ys = half_sum_dpp(omega * xv);
        if (node == 0) ym[t] = pass ? ym[t] + ys : ys;
        if (exact) zm[t] = xv;
      }
    }
    }  // pass
  }
  __syncthreads();
  // rows l (slot 0) and J0 + l (slot 1) in walk order: side 1 walks KP-1 .. H
  auto walk = [](int i) { return i < H ? i : H + (KP - 1 - i); };
  const int w0 = walk(mem0 ? l : 0), w1 = walk(J0 + l);
  double y0 = mem0 ? sm.Ym[w0] : 0.0, y1 = sm.Ym[w1];
  const double d = wave_sum_dpp(fma(mem0 ? sm.tq[l][2] : 0.0, sm.Zm[w0],
                                    sm.tq[J0 + l][2] * sm.Zm[w1]));
  if (CWBL_DBG_STOP(c) == 3) {  // timing ablation: stop after the quadrature
    if (INFO && l == 0) info[gi] = make_int2(ptot, (int)(d + y0 + y1));
    return;
  }

  // ---- back-transform y <- Q y = H_0 H_1 ... H_{k-3} y, four reflectors per reduction ------
  auto apply4 = [&](const double (&v0)[4], const double (&v1)[4], const double (&ta)[4]) {
    double t[12];
    sfor<4>([&](auto qq) { t[qq] = fma(v0[qq], y0, v1[qq] * y1); });
    constexpr int PP[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    sfor<6>([&](auto ee) {
      constexpr int a = PP[ee][0], b = PP[ee][1];
      t[4 + ee] = fma(v0[a], v0[b], v1[a] * v1[b]);
    });
    t[10] = t[11] = 0.0;
    wave_sum4_dpp(t[0], t[1], t[2], t[3]);
    wave_sum4_dpp(t[4], t[5], t[6], t[7]);
    wave_sum4_dpp(t[8], t[9], t[10], t[11]);
    // t: d0..d3, G01 G02 G03 G12 G13 G23
    const double c3 = ta[3] * t[3];
    const double c2 = ta[2] * fma(-c3, t[9], t[2]);
    const double c1 = ta[1] * fma(-c3, t[8], fma(-c2, t[7], t[1]));
    const double c0 = ta[0] * fma(-c3, t[6], fma(-c2, t[5], fma(-c1, t[4], t[0])));
    y0 = fma(-c0, v0[0], fma(-c1, v0[1], fma(-c2, v0[2], fma(-c3, v0[3], y0))));
    y1 = fma(-c0, v1[0], fma(-c1, v1[1], fma(-c2, v1[2], fma(-c3, v1[3], y1))));
  };
  // the groups run as a static pipeline over a ring of register slots holding the raw loaded
  // rows only (solve_tqb_tail_kernel's: the wait before a group covers only its own loads)
  auto issue_tail = [&](int top, double (&x)[4]) {
    sfor<4>([&](auto qq) {
      const int jl = top - 3 + qq;  // < 0: padding (H = I)
      x[qq] = ld_tail(jl, jl >= 0 && l > jl + 1);
    });
  };
  auto form_tail = [&](int top, const double (&x)[4], double (&v1)[4], double (&ta)[4]) {
    sfor<4>([&](auto qq) {
      const int jl = top - 3 + qq, jc = jl < 0 ? 0 : jl;
      const int j1 = jl + 1;
      const double pad = jl < 0 ? 0.0 : 1.0;  // padding group entries: H = I
      const double sc = sm.scl[J0 + jc];
      v1[qq] = pad * (l == j1 ? 1.0 : (l > j1 ? sc * x[qq] : 0.0));
      ta[qq] = pad * sm.tau[J0 + jc];
    });
  };
  auto issue_hand = [&](auto TOP, double (&x0)[4], double (&x1)[4]) {
    sfor<4>([&](auto qq) {
      constexpr int j = decltype(TOP)::value - 3 + decltype(qq)::value;
      ld_hand(std::integral_constant<int, j>{}, x0[qq], x1[qq]);
    });
  };
  {
    constexpr int NGT = (KT - 2 + 3) / 4;  // groups of the tail's reflectors at k = KP
    constexpr int D = NGT < 8 ? NGT : 8;   // groups in flight (8 VGPRs each)
    const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
    double rx[D][4];
    sfor<D>([&](auto G) { issue_tail(nst - 1 - 4 * decltype(G)::value, rx[decltype(G)::value]); });
    sfor<NGT>([&](auto G) {
      constexpr int g = decltype(G)::value, sl = g % D;
      double v1[4], ta[4];
      form_tail(nst - 1 - 4 * g, rx[sl], v1, ta);
      if constexpr (g + D < NGT) issue_tail(nst - 1 - 4 * (g + D), rx[sl]);
      apply4(zero4, v1, ta);
    });
  }
  {
    constexpr int NGH = J0 / 4;            // the hand-off's reflectors (rows > j)
    constexpr int D = NGH < 4 ? NGH : 4;   // (v0 and v1: 16 VGPRs each)
    double r0[D][4], r1[D][4];
    sfor<D>([&](auto G) {
      constexpr int g = decltype(G)::value;
      issue_hand(std::integral_constant<int, J0 - 1 - 4 * g>{}, r0[g], r1[g]);
    });
    sfor<NGH>([&](auto G) {
      constexpr int g = decltype(G)::value, sl = g % D, top = J0 - 1 - 4 * g;
      double v0[4], v1[4], ta[4];
      sfor<4>([&](auto qq) {
        v0[qq] = r0[sl][qq];
        v1[qq] = r1[sl][qq];
        ta[qq] = sm.tau[top - 3 + decltype(qq)::value];
      });
      if constexpr (g + D < NGH)
        issue_hand(std::integral_constant<int, J0 - 1 - 4 * (g + D)>{}, r0[sl], r1[sl]);
      apply4(v0, v1, ta);
    });
  }

  // ---- analysis and RTPP / RTPS (:671-698), fp32 in the reference's order -----------------
  // sequential fp32 sum over members 0 .. k-1 (member m: slot m / J0, lane m % J0)
  auto seq_sum_f32 = [&](float a0, float a1) {
    float s = 0.0f;
    for (int mm = 0; mm < J0; ++mm) s = s + readlane_f32(a0, mm);
    for (int mm = J0; mm < k; ++mm) s = s + readlane_f32(a1, mm - J0);
    return s;
  };
  const double xb_mean = (double)(seq_sum_f32(xb0, xb1) * c.nmember_inv);  // fp32 (:671)
  const double sk = sqrt((double)(k - 1));
  float xa0 = (float)(xb_mean + (d + sk * y0));
  float xa1 = mem1 ? (float)(xb_mean + (d + sk * y1)) : 0.0f;
  if (c.use_rtpp || c.use_rtps) {
    const float xa_mean = seq_sum_f32(xa0, xa1) * c.nmember_inv;
    const double xp0 = (double)xb0 - xb_mean;
    const double xp1 = mem1 ? (double)xb1 - xb_mean : 0.0;
    float xap0 = xa0 - xa_mean;
    float xap1 = mem1 ? xa1 - xa_mean : 0.0f;
    if (c.use_rtpp) {
      xap0 = (float)((double)((1.0f - c.rtpp_alpha) * xap0) + (double)c.rtpp_alpha * xp0);
      if (mem1)
        xap1 = (float)((double)((1.0f - c.rtpp_alpha) * xap1) + (double)c.rtpp_alpha * xp1);
    }
    if (c.use_rtps) {
      double d8 = 0.0;
      for (int mm = 0; mm < J0; ++mm) {
        const double xp = readlane_f64(xp0, mm);
        d8 = d8 + xp * xp;
      }
      for (int mm = J0; mm < k; ++mm) {
        const double xp = readlane_f64(xp1, mm - J0);
        d8 = d8 + xp * xp;
      }
      const float xb_std = (float)d8;
      const float xa_std = seq_sum_f32(xap0 * xap0, xap1 * xap1);
      const float f = c.rtps_alpha * sqrtf(xb_std / xa_std) - c.rtps_alpha + 1.0f;
      xap0 = xap0 * f;
      xap1 = xap1 * f;
    }
    xa0 = xa_mean + xap0;
    xa1 = xa_mean + xap1;
  }
  if (mem0) slab.var[P + slab.L * l] = xa0;
  if (mem1) slab.var[P + slab.L * (J0 + l)] = xa1;
  // info.y: decade of the quadrature rule (negative when M/m exceeds the last table)
  if (INFO && l == 0) info[gi] = make_int2(ptot, ratio > dec ? -level : level);
}

// The hit's body, from the background's loads to the stores: point gi of the launch (its factor
// at fac + gi WORDS, its accepted count ptot) analysed at var index P (member 0).  sm is the workgroup's
// own; a caller that runs it again (a further level of a column) puts a barrier between.
// INFO: info[gi] is stored, as the hit kernel does; a level of a column stores none.
template <int KP, int J0, bool INFO = true>
__device__ __forceinline__ void tqb_factor_hit(TailSmem<KP, J0> &sm, const SolveConsts &c,
                                               const SlabDev &slab, int gi, int l, int k,
                                               long long P, const double *__restrict__ fac,
                                               int ptot, int2 *__restrict__ info) {
  using F = BigFactor<KP, J0>;
  constexpr int KT = KP - J0;
  constexpr int NS = KT - 2;  // the tail's steps at k = KP
  static_assert(KT == 64 && KP > 64 && KP - 64 <= J0 && NS <= 2 * (J0 - 1),
                "rows 64 .. KP-1 on the prefix lanes; two tail columns behind each head step");
  const bool mem0 = l < J0;      // prefix row / member l exists (k > J0)
  const bool mem1 = J0 + l < k;  // member J0 + l exists
  const bool memh = 64 + l < k;  // member 64 + l exists (the hand-off kernel's wave 1)
  // the background in the tail's layout (members l and J0 + l) and, for the replay of the
  // hand-off kernel's steps, in its layout (members l and 64 + l)
  const float xb0v = slab.var[P + slab.L * (mem0 ? l : 0)];  // branch-free: valid addresses
  const float xb1v = slab.var[P + slab.L * (mem1 ? J0 + l : 0)];
  const float xh0v = slab.var[P + slab.L * l];  // k > 64
  const float xh1v = slab.var[P + slab.L * (memh ? 64 + l : 0)];
  __builtin_amdgcn_sched_barrier(0);
  const float xb0 = mem0 ? xb0v : 0.0f;
  const float xb1 = mem1 ? xb1v : 0.0f;

  const auto frs = rec_rsrc(fac + (long long)gi * F::WORDS, F::WORDS);
  const unsigned l8 = 8u * (unsigned)l;
  // word W + l of the factor (W constant: the scalar offset of the load)
  auto ldw = [&](auto W) {
    constexpr int wd = decltype(W)::value;
    static_assert(wd >= 0 && wd + 63 < F::WORDS, "every lane's word lies in the point's factor");
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(frs, (int)l8, 8 * wd, 0);
    return __longlong_as_double(((long long)v[1] << 32) | (unsigned)v[0]);
  };
  using std::integral_constant;
  const double tauh = ldw(integral_constant<int, F::TAU>{});        // tau_l: steps < 64
  const double taut = ldw(integral_constant<int, F::TAU + J0>{});   // tau_{J0 + l}
  const double sclt = ldw(integral_constant<int, F::SCAL + J0>{});  // scal_{J0 + l}
  __builtin_amdgcn_sched_barrier(0);
  double h0[J0], h1[J0];  // reflector j: rows l and 64 + l
  sfor<J0>([&](auto J) {
    constexpr int j = decltype(J)::value;
    h0[j] = ldw(integral_constant<int, F::hv(j) - (j + 1)>{});
    h1[j] = ldw(integral_constant<int, F::hv(j) - (j + 1) + 64>{});
    __builtin_amdgcn_sched_barrier(0);
  });
  double t[NS];  // the tail's column jl: row J0 + l

  // xb_mean = sum(xb) * nmember_inv in fp32 (:671), sequential like the reference (the hand-off
  // kernel sums the members in the same order)
  float xs = 0.0f;
  for (int mm = 0; mm < J0; ++mm) xs = xs + readlane_f32(xb0, mm);
  for (int mm = J0; mm < k; ++mm) xs = xs + readlane_f32(xb1, mm - J0);
  const double xb_mean = (double)(xs * c.nmember_inv);
  double ux0 = (double)xh0v - xb_mean;                 // x' of rows l (l < 64 < k)
  double ux1 = memh ? (double)xh1v - xb_mean : 0.0;    // x' of rows 64 + l, zeros past k

  // ---- steps j < J0: the hand-off kernel's x' half --------------------------------------
  sfor<J0>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const double tau = readlane_f64(tauh, j);
    const double v0 = l > j ? h0[j] : 0.0;          // v = 0 at rows <= j, 1 at row j + 1
    const double v1 = l < KP - 64 ? h1[j] : 0.0;
    double z0 = 0.0, p0 = v0 * ux0, p1 = v1 * ux1, z3 = 0.0;
    wave_sum4_dpp(z0, p0, p1, z3);
    const double s2 = (p0 + p1) + (0.0 + 0.0);  // bsum4: (w0 + w1) + (w2 + w3)
    ux0 = fma(-tau * s2, v0, ux0);
    ux1 = fma(-tau * s2, v1, ux1);
    if constexpr (2 * j < NS) {
      t[2 * j] = ldw(integral_constant<int, F::bt(2 * j) - (2 * j + 2)>{});
      if constexpr (2 * j + 1 < NS)
        t[2 * j + 1] = ldw(integral_constant<int, F::bt(2 * j + 1) - (2 * j + 3)>{});
      __builtin_amdgcn_sched_barrier(0);
    }
  });
  // what only the solve reads: rows l and 64 + l of T and Q^T b1
  const double dv0 = ldw(integral_constant<int, F::D>{});
  const double dv1 = ldw(integral_constant<int, F::D + 64>{});
  const double cv0 = ldw(integral_constant<int, F::C>{});
  const double cv1 = ldw(integral_constant<int, F::C + 64>{});
  const double uv0 = ldw(integral_constant<int, F::U1>{});
  const double uv1 = ldw(integral_constant<int, F::U1 + 64>{});
  __builtin_amdgcn_sched_barrier(0);

  // ---- to the tail's layout: lane l takes row J0 + l (through LDS, as the tail loads U2) ---
  sm.Ym[l] = ux0;
  if (l < KP - 64) sm.Ym[64 + l] = ux1;
  __syncthreads();
  double u2t = sm.Ym[J0 + l];
  if (mem0) sm.tq[l][3] = ux0;
  const int nst = k - 2 - J0;  // k > J0 + 2 (launcher)

  // ---- steps j = J0 .. k-3: the tail's x' half ---------------------------------------------
  sfor<NS>([&](auto JL) {
    constexpr int jl = decltype(JL)::value, j1 = jl + 1;
    if (jl < nst) {  // (uniform)
      const double tau = readlane_f64(taut, jl), scal = readlane_f64(sclt, jl);
      const double x = l > j1 ? t[jl] : 0.0;
      // the tail's slot of wave_sum4_dpp (the sum's bits do not depend on it; a NaN's might)
      double z0 = 0.0, xu = x * u2t, z2 = 0.0, z3 = 0.0;
      wave_sum4_dpp(z0, xu, z2, z3);
      const double v = l == j1 ? 1.0 : x * scal;
      const double s2 = fma(scal, xu, readlane_f64(u2t, j1));  // v . x'
      u2t = fma(-tau * s2, v, u2t);
    }
  });

  // sm.tq, sm.tau and sm.scl as the tail's loop leaves them
  sm.tq[l][0] = dv0;
  sm.tq[l][1] = cv0;
  sm.tq[l][2] = uv0;
  sm.tau[l] = tauh;
  if (l < KP - 64) {
    sm.tq[64 + l][0] = dv1;
    sm.tq[64 + l][1] = cv1;
    sm.tq[64 + l][2] = uv1;
  }
  sm.tau[J0 + l] = taut;
  sm.scl[J0 + l] = sclt;
  sm.tq[J0 + l][3] = u2t;
  if (l == 0) sm.tq[KP][1] = 0.0;
  __syncthreads();
  // trace A = d_0 + d_1 + ... + d_{k-1}, added in the kernel pair's order
  double trace = 0.0;
  for (int j = 0; j < k; ++j) trace += sm.tq[j][0];

  tqb_finish<KP, J0, INFO>(
      sm, c, slab, gi, l, k, P, xb0, xb1, mem0, mem1, trace, ptot, info,
      [&](int jl, bool live) {
        // (jl < 0 on a padding group: not live)
        return rec_ld(frs, rec_off(live, F::bt(jl) + l - (jl + 2)));
      },
      [&](auto J, double &x0, double &x1) {
        constexpr int j = decltype(J)::value;
        x0 = rec_ld(frs, rec_off(mem0 && l > j, F::hv(j) + l - (j + 1)));
        x1 = rec_ld(frs, 8u * (unsigned)(F::hv(j) + J0 + l - (j + 1)));
      });
}

// The body of a level kernel of a column-shared call, with the first level as an argument: the
// levels kzf + lw blockIdx.y .. of column blockIdx.x (through xcd_remap_rev) from the
// BigFactor<KP, J0> at fac + gi WORDS, each one tqb_factor_hit at the level's var index.
// cwbl_tq_big_column_all.hip calls it with kzf = 0 (every level of a column whose factor the
// column cache kept, CWBL_OPT_COLUMN_REUSE).  It is the text of solve_tqb_factor_column_kernel
// (cwbl_tq_big_column.hip), which starts at level 1 and keeps its own copy: as a caller of this
// function that kernel compiles to another schedule (profiles/column_reuse.txt), and its assembly
// is not to change.  sm is the workgroup's own; info is read only.
template <int KP, int J0>
__device__ __forceinline__ void tqb_factor_levels(TailSmem<KP, J0> &sm, const SolveConsts &c,
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
    tqb_factor_hit<KP, J0, false>(sm, c, slab, gi, ll, k, P0 + nxy * kz, fp, ptot, nullptr);
  }
}

}  // namespace

// solve_tqb_tail_kernel<KP, J0, 2> (see there for the step's derivation) with the factor's
// stores.  fac: the BigFactor of point gi of the launch at fac + gi WORDS; a point with p = 0
// writes none (a hit leaves at its info).
// (two waves per SIMD at KP = 128 as well, where the tail has three: 219 VGPRs and no scratch;
// bounded to 168 it spills 24 VGPRs to 100 B of scratch)
template <int KP, int J0>
__global__ void __launch_bounds__(64, 2)
fill_tqb_tail_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                     double *__restrict__ ws, int2 *__restrict__ info, double *__restrict__ fac) {
  using HO = BigHandoff<KP, J0>;
  using F = BigFactor<KP, J0>;
  constexpr int KT = HO::KT;  // trailing rows: one per lane
  constexpr int NG = KT / 8;  // column groups
  static_assert(KT == 64 && J0 <= 64 && J0 % 4 == 0, "one trailing row per lane; prefix rows on lanes < J0");
  using SM = TailSmem<KP, J0>;
  __shared__ SM sm;

  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);
  if (gi >= npts) return;
  const int l = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var unchanged (:220, :226)
  const auto *__restrict__ w = gptr(ws + (long long)gi * HO::WORDS);

  const long long P = bf_point_index(slab, g0 + gi);
  const bool mem0 = l < J0;      // prefix row / member l exists (k > J0)
  const bool mem1 = J0 + l < k;  // member J0 + l exists
  const float xb0v = slab.var[P + slab.L * (mem0 ? l : 0)];  // branch-free: valid addresses
  const float xb1v = slab.var[P + slab.L * (mem1 ? J0 + l : 0)];
  const float xb0 = mem0 ? xb0v : 0.0f;
  const float xb1 = mem1 ? xb1v : 0.0f;

  // ---- hand-off: trailing rows (coalesced by column), T and the vectors' prefix ----------
  double A[KT];
  sfor<KT>([&](auto cc) {
    constexpr int col = decltype(cc)::value;
    A[col] = w[HO::TA + col * KT + l];
  });
  double u1t = w[HO::U1 + J0 + l], u2t = w[HO::U2 + J0 + l];  // trailing Q^T b1, Q^T x'
  if (mem0) {
    sm.tq[l][0] = w[HO::D + l];
    sm.tq[l + 1][1] = w[HO::E + l];
    sm.tq[l][2] = w[HO::U1 + l];
    sm.tq[l][3] = w[HO::U2 + l];
    sm.tau[l] = w[HO::TAU + l];
  }
  // trailing rows of T: decoupled unit rows until the steps write them (rows >= k stay so)
  sm.tq[J0 + l][0] = 1.0;
  sm.tq[J0 + l + 1][1] = 0.0;
  sm.tau[J0 + l] = 0.0;
  sm.scl[J0 + l] = 0.0;  // (the factor keeps no unwritten LDS; nothing reads the rows past k-3)
  if (l == 0) sm.tq[0][1] = 0.0;
  __syncthreads();
  double trace = 0.0;  // d_0 + d_1 + ... in step order, as solve_tq_big_kernel sums it
  for (int j = 0; j < J0; ++j) trace += sm.tq[j][0];

  // lane jl's row -> sm.row (static register indices): the trailing 2x2 block's entries
  auto publish_row = [&](int jl) {
    __syncthreads();  // the previous readers of sm.row are done
    if (l == jl) {
      sfor<KT / 2>([&](auto cc) {
        constexpr int col = 2 * decltype(cc)::value;
        *reinterpret_cast<double2 *>(&sm.row[col]) = make_double2(A[col], A[col + 1]);
      });
    }
    __syncthreads();
  };
  const auto rec = rec_rsrc(ws + (long long)gi * HO::WORDS, HO::WORDS);
  const auto frs = rec_rsrc(fac + (long long)gi * F::WORDS, F::WORDS);  // the point's factor

  // ---- Householder steps j = J0 .. k-3 (local jl = j - J0) --------------------------------
  auto rep4 = [](double x, double (&R)[4]) {
    const int xl = (int)__double_as_longlong(x), xh = (int)(__double_as_longlong(x) >> 32);
    auto mk = [](int lo, int hi) {
      return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
    };
    // rows (0, 1, 0, 1) and (2, 3, 2, 3), then each row of those over its pair
    const auto al = __builtin_amdgcn_permlane32_swap(xl, xl, false, false);
    const auto ah = __builtin_amdgcn_permlane32_swap(xh, xh, false, false);
    const auto bl = __builtin_amdgcn_permlane16_swap(al[0], al[0], false, false);
    const auto bh = __builtin_amdgcn_permlane16_swap(ah[0], ah[0], false, false);
    const auto cl = __builtin_amdgcn_permlane16_swap(al[1], al[1], false, false);
    const auto ch = __builtin_amdgcn_permlane16_swap(ah[1], ah[1], false, false);
    R[0] = mk(bl[0], bh[0]);
    R[1] = mk(bl[1], bh[1]);
    R[2] = mk(cl[0], ch[0]);
    R[3] = mk(cl[1], ch[1]);
    // a DPP source is not read within two wait states of its VALU write
    asm volatile("s_nop 1" : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3]));
  };
  const int nst = k - 2 - J0;  // k > J0 + 2 (launcher)
  auto step = [&](auto GB, int jl) {
    constexpr int gb = decltype(GB)::value;
    constexpr int jb = gb == 0 ? 0 : 8 * gb - 1;  // the block's first step
    const int j = J0 + jl, j1 = jl + 1;
    auto opq = [](double a) {
      asm("" : "+v"(a));
      return a;
    };
    double xr = opq(A[jb]);
    sfor<7>([&](auto ii) {
      constexpr int cc = jb + 1 + decltype(ii)::value;
      if constexpr (cc < KT) xr = jl == cc ? opq(A[cc]) : xr;
    });
    rec_st(rec, rec_off(l > j1, HO::BT + jl * KT + l), xr);
    // the factor's column: the same rows, packed
    rec_st(frs, rec_off(l > j1, F::bt(jl) + l - (jl + 2)), xr);
    const double dj = readlane_f64(xr, jl), alpha = readlane_f64(xr, j1);
    trace += dj;
    const double x = l > j1 ? xr : 0.0;
    double xx = x * x, xu = x * u2t, xb = x * u1t, z3 = 0.0;
    wave_sum4_dpp(xx, xu, xb, z3);
    // dlarfg with fp64 rcp/rsq refined to ~1 ulp; H = I when x = 0 (tau = 0, v = e_j+1)
    const double a2 = fma(alpha, alpha, xx);
    const double rs = rsq64(a2);  // 1/|beta|
    const bool nz = xx > 0.0;
    const double bt = -copysign(a2 * rs, alpha);
    const double beta = nz ? bt : alpha;
    const double tau = nz ? (bt - alpha) * -copysign(rs, alpha) : 0.0;
    const double rab = rcp64(alpha - bt);
    const double scal = nz ? rab : 0.0;
    if (l == 0) {
      sm.tq[j][0] = dj;
      sm.tq[j + 1][1] = beta;
      sm.tau[j] = tau;
      sm.scl[j] = scal;
    }
    const double v = l == j1 ? 1.0 : x * scal;
    const double s2 = fma(scal, xu, readlane_f64(u2t, j1));  // v . x'
    const double s3 = fma(scal, xb, readlane_f64(u1t, j1));  // v . b1
    u2t = fma(-tau * s2, v, u2t);
    u1t = fma(-tau * s3, v, u1t);
    const double amb = nz ? alpha - bt : 0.0;
    double R[4], W[4];
    rep4(l > j1 ? x : l == j1 ? amb : 0.0, R);
    // A v = scal * sum_{c >= j+1} A(:, c) xt_c (volatile forms, in this order)
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    sfor<KT - 8 * gb>([&](auto cc) {
      constexpr int col = 8 * gb + decltype(cc)::value;
      q[col % 4] = fmac_row_v<col % 16>(q[col % 4], R[col / 16], A[col]);
    });
    const double av = scal * ((q[0] + q[1]) + (q[2] + q[3]));  // (A v)_l
    const double s1 = tau * wave_sum_dpp(v * av);   // v^T (tau A v); v = 0 at rows <= j
    const double wl = fma(-0.5 * tau * s1, v, tau * av);
    const double wsl = wl * scal;
    rep4(wl, W);
    // A <- A - w v^T - v w^T, a group's eight columns per pass
    sfor<NG - gb>([&](auto gg) {
      constexpr int c0 = 8 * (gb + decltype(gg)::value);
      sfor<8>([&](auto ii) {
        constexpr int col = c0 + decltype(ii)::value;
        A[col] = fnmac_row_v<col % 16>(A[col], R[col / 16], wsl);
      });
      sfor<8>([&](auto ii) {
        constexpr int col = c0 + decltype(ii)::value;
        A[col] = fnmac_row_v<col % 16>(A[col], W[col / 16], v);
      });
    });
  };
  const int nrun = CWBL_DBG_STOP(c) == 2 && CWBL_DBG_STEPS(c) > 64 ? min(nst, CWBL_DBG_STEPS(c) - 64) : nst;
  sfor<NG>([&](auto GB) {  // block gb: steps jl = 8 gb - 1 .. 8 gb + 6 (column j + 1 in group gb)
    constexpr int gb = decltype(GB)::value;
    const int hi = min(8 * gb + 6, nrun - 1);
    for (int jl = gb == 0 ? 0 : 8 * gb - 1; jl <= hi; ++jl) step(GB, jl);
  });
  {  // the trailing 2x2 (rows k-2, k-1): already tridiagonal
    const int jl = nst;
    publish_row(jl);
    const double d0 = sm.row[jl], e1 = sm.row[jl + 1];
    publish_row(jl + 1);
    const double d1 = sm.row[jl + 1];
    trace += d0;
    trace += d1;
    if (l == 0) {
      sm.tq[k - 2][0] = d0;
      sm.tq[k - 1][1] = e1;
      sm.tq[k - 1][0] = d1;
    }
  }
  sm.tq[J0 + l][2] = u1t;
  sm.tq[J0 + l][3] = u2t;
  __syncthreads();
  if (CWBL_DBG_STOP(c) == 2) {  // timing ablation: stop after the tridiagonalisation
    if (l == 0) info[gi] = make_int2(ptot, (int)(trace + u1t + u2t));
    return;
  }
  // the factor's five arrays as the loop left them: rows l, and 64 + l on the lanes that have one
  {
    const bool up = 64 + l < KP;
    const int lu = up ? 64 + l : 0;
    rec_st(frs, 8u * (F::D + l), sm.tq[l][0]);
    rec_st(frs, rec_off(up, F::D + lu), sm.tq[lu][0]);
    rec_st(frs, 8u * (F::C + l), sm.tq[l][1]);
    rec_st(frs, rec_off(up, F::C + lu), sm.tq[lu][1]);
    rec_st(frs, 8u * (F::U1 + l), sm.tq[l][2]);
    rec_st(frs, rec_off(up, F::U1 + lu), sm.tq[lu][2]);
    rec_st(frs, 8u * (F::TAU + l), sm.tau[l]);
    rec_st(frs, rec_off(up, F::TAU + lu), sm.tau[lu]);
    rec_st(frs, 8u * (F::SCAL + J0 + l), sm.scl[J0 + l]);
  }
  tqb_finish<KP, J0>(
      sm, c, slab, gi, l, k, P, xb0, xb1, mem0, mem1, trace, ptot, info,
      [&](int jl, bool live) { return rec_ld(rec, rec_off(live, HO::BT + jl * KT + l)); },
      [&](auto J, double &x0, double &x1) {
        constexpr int j = decltype(J)::value;
        // rows <= j hold zeros (not loaded); row j + 1 holds 1.0
        x0 = rec_ld(rec, rec_off(mem0 && l > j, HO::HV + j * KP + l));
        x1 = w[HO::HV + j * KP + J0 + l];
        // the factor's reflector j: rows j + 1 .. KP-1 as the hand-off kernel left them
        rec_st(frs, rec_off(mem0 && l > j, F::hv(j) + l - (j + 1)), x0);
        rec_st(frs, 8u * (F::hv(j) + J0 + l - (j + 1)), x1);
      });
}

// The hit kernel: cwbl_tq_big_factor.hip defines it (KP = 96), cwbl_tq_rows_factor.hip
// specialises it at <128, 64>.
template <int KP, int J0>
__global__ void solve_tqb_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                                        const double *__restrict__ fac,
                                        int2 *__restrict__ info);

}  // namespace cwbl
