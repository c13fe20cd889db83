// cwbl_tq_rows_factor.h — the half-row hit's body (KP = 128, k = 97..128) as a function:
// solve_tqb_factor_kernel<128, 64> (cwbl_tq_rows_factor.hip, CWBL_OPT_ROWS_REUSE) calls it once,
// the level kernels of a column-shared call (cwbl_tq_rows_column.hip, CWBL_OPT_COLUMN_ROWS) once
// per level.  The hit kernel's assembly equals the parent's in every line with its body here
// (profiles/column_rows.txt), as tqb_factor_hit left the <96, 32> hit kernel's.
#pragma once

#include "cwbl_tq_big_factor.h"

namespace cwbl {

namespace {

// The reflectors the hit's ring holds (two registers each; a slot that the last reflectors leave
// takes two of the tail's columns).
constexpr int kRowsHitRing = 16;

// The hit's body, from the background's loads to the stores: point gi of the launch (its
// BigFactor<128, 64> at fac + gi WORDS, its accepted count ptot) analysed at var index P
// (member 0).  sm is the workgroup's own; a caller that runs it again (a further level of a
// column) puts a barrier between.  INFO: info[gi] is stored, as the hit kernel does; a level of a
// column stores none.
//
// Lane l holds rows l and 64 + l in both halves of the replay: the half-row kernel's waves 0 and
// 2 hold x' so, and with J0 = 64 it is the tail's layout as well.  The loads are unconditional,
// each a constant offset from one lane offset into the point's own factor (a load under a lane
// mask is a branch of its own, and the waits behind such branches come out as vmcnt(0)); the row
// mask is applied at the use.  They are issued in the order of first use: the scalars and the
// first DH reflectors before step 0, reflector j + DH behind step j, two of the tail's columns
// behind each of the last DH replayed steps, the rest of them one behind each of the tail's
// steps, T and Q^T b1 last.  With 2 DH + 5 loads in flight at most the waits count down within
// vmcnt's 63.
template <bool INFO>
__device__ __forceinline__ void tqb_rows_hit(TailSmem<128, 64> &sm, const SolveConsts &c,
                                             const SlabDev &slab, int gi, int l, int k,
                                             long long P, const double *__restrict__ fac,
                                             int ptot, int2 *__restrict__ info) {
  constexpr int KP = 128, J0 = 64;
  using F = BigFactor<KP, J0>;
  constexpr int KT = KP - J0;
  constexpr int NS = KT - 2;  // the tail's steps at k = KP
  constexpr int DH = kRowsHitRing;
  static_assert(KP == 128 && J0 == 64 && KT == 64, "rows l and 64 + l of both halves on lane l");
  static_assert(DH >= 1 && DH <= J0 && 2 * DH <= NS && 2 * DH + 5 <= 63,
                "the ring's columns and the loads in flight");
  const bool mem1 = J0 + l < k;  // member 64 + l exists (k > 64: member l does)
  const float xb0 = slab.var[P + slab.L * l];
  const float xb1v = slab.var[P + slab.L * (mem1 ? J0 + l : 0)];  // branch-free: a valid address
  __builtin_amdgcn_sched_barrier(0);
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
  const double taut = ldw(integral_constant<int, F::TAU + J0>{});   // tau_{64 + l}
  const double sclt = ldw(integral_constant<int, F::SCAL + J0>{});  // scal_{64 + l}
  __builtin_amdgcn_sched_barrier(0);
  // The ring: every element is written by one load and read by one step, so the registers of a
  // column are free once its step has run, and the loads below take them in that order.
  double h0[J0], h1[J0];  // reflector j: rows l and 64 + l
  double t[NS];           // the tail's column jl: row 64 + l
  double dv0, dv1, cv0, cv1, uv0, uv1;  // rows l and 64 + l of T and Q^T b1
  auto issue_head = [&](auto J) {
    constexpr int j = decltype(J)::value;
    h0[j] = ldw(integral_constant<int, F::hv(j) - (j + 1)>{});
    h1[j] = ldw(integral_constant<int, F::hv(j) - (j + 1) + 64>{});
  };
  auto issue_tail = [&](auto JL) {
    constexpr int jl = decltype(JL)::value;
    if constexpr (jl < NS) t[jl] = ldw(integral_constant<int, F::bt(jl) - (jl + 2)>{});
  };
  auto issue_t = [&]() {  // what only the solve reads
    dv0 = ldw(integral_constant<int, F::D>{});
    dv1 = ldw(integral_constant<int, F::D + 64>{});
    cv0 = ldw(integral_constant<int, F::C>{});
    cv1 = ldw(integral_constant<int, F::C + 64>{});
    uv0 = ldw(integral_constant<int, F::U1>{});
    uv1 = ldw(integral_constant<int, F::U1 + 64>{});
  };
  sfor<DH>([&](auto J) {
    issue_head(J);
    __builtin_amdgcn_sched_barrier(0);
  });

  // xb_mean = sum(xb) * nmember_inv in fp32 (:671), sequential like the reference (the half-row
  // kernel sums the members in the same order)
  float xs = 0.0f;
  for (int mm = 0; mm < J0; ++mm) xs = xs + readlane_f32(xb0, mm);
  for (int mm = J0; mm < k; ++mm) xs = xs + readlane_f32(xb1, mm - J0);
  const double xb_mean = (double)(xs * c.nmember_inv);
  double ux0 = (double)xb0 - xb_mean;               // x' of rows l
  double ux1 = mem1 ? (double)xb1v - xb_mean : 0.0;  // x' of rows 64 + l, zeros past k

  // ---- steps j < 64: solve_tq_rows_kernel's x' half -------------------------------------------
  // Its wave 0 sums v . x' over rows l, its wave 2 over rows 64 + l, waves 1 and 3 (the other
  // column half) sum zeros; then su = (redB[0] + redB[1]) + (redB[2] + redB[3]).  The additions
  // of +0.0 stay: -0.0 + 0.0 is not -0.0.  There is no early exit: a step with tau = 0 runs
  // its expressions.
  sfor<J0>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const double tau = readlane_f64(tauh, j);
    const double v0 = l > j ? h0[j] : 0.0;  // v = 0 at rows <= j, 1 at row j + 1
    const double v1 = h1[j];                // rows >= 64 are all live
    double z0 = 0.0, p0 = v0 * ux0, p1 = v1 * ux1, z3 = 0.0;
    wave_sum4_dpp(z0, p0, p1, z3);  // (a sum's bits do not depend on its slot)
    const double su = (p0 + 0.0) + (p1 + 0.0);
    ux0 = fma(-tau * su, v0, ux0);
    ux1 = fma(-tau * su, v1, ux1);
    if constexpr (j + DH < J0) {
      issue_head(integral_constant<int, j + DH>{});
    } else {
      issue_tail(integral_constant<int, 2 * (j + DH - J0)>{});
      issue_tail(integral_constant<int, 2 * (j + DH - J0) + 1>{});
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  if constexpr (2 * DH >= NS) {
    issue_t();
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- the tail's layout is this one (J0 = 64): lane l keeps row 64 + l ---------------------
  double u2t = ux1;
  sm.tq[l][3] = ux0;
  const int nst = k - 2 - J0;  // k > J0 + 2 (launcher)

  // ---- steps j = 64 .. k-3: the tail's x' half ------------------------------------------------
  sfor<NS>([&](auto JL) {
    constexpr int jl = decltype(JL)::value, j1 = jl + 1;
    // A step past k-3 (k < KP) runs on whatever its column's words hold and is dropped by a
    // select, not skipped by a branch: the load of the first column that only a branch reads
    // sinks to that use and waits there for everything in flight.
    {
      const double tau = readlane_f64(taut, jl), scal = readlane_f64(sclt, jl);
      const double x = l > j1 ? t[jl] : 0.0;
      // the tail's slot of wave_sum4_dpp
      double z0 = 0.0, xu = x * u2t, z2 = 0.0, z3 = 0.0;
      wave_sum4_dpp(z0, xu, z2, z3);
      const double v = l == j1 ? 1.0 : x * scal;
      const double s2 = fma(scal, xu, readlane_f64(u2t, j1));  // v . x'
      const double un = fma(-tau * s2, v, u2t);
      u2t = jl < nst ? un : u2t;  // (uniform)
    }
    if constexpr (jl + 2 * DH < NS) {
      issue_tail(integral_constant<int, jl + 2 * DH>{});
      if constexpr (jl + 2 * DH == NS - 1) issue_t();
      __builtin_amdgcn_sched_barrier(0);
    }
  });

  // sm.tq, sm.tau and sm.scl as the tail's loop leaves them
  sm.tq[l][0] = dv0;
  sm.tq[l][1] = cv0;
  sm.tq[l][2] = uv0;
  sm.tau[l] = tauh;
  sm.tq[64 + l][0] = dv1;
  sm.tq[64 + l][1] = cv1;
  sm.tq[64 + l][2] = uv1;
  sm.tau[J0 + l] = taut;
  sm.scl[J0 + l] = sclt;
  sm.tq[J0 + l][3] = u2t;
  if (l == 0) sm.tq[KP][1] = 0.0;
  __syncthreads();
  // trace A = d_0 + d_1 + ... + d_{k-1}, added in the kernel pair's order
  double trace = 0.0;
  for (int j = 0; j < k; ++j) trace += sm.tq[j][0];

  tqb_finish<KP, J0, INFO>(
      sm, c, slab, gi, l, k, P, xb0, xb1, true, mem1, trace, ptot, info,
      [&](int jl, bool live) {
        // (jl < 0 on a padding group: not live)
        return rec_ld(frs, rec_off(live, F::bt(jl) + l - (jl + 2)));
      },
      [&](auto J, double &x0, double &x1) {
        constexpr int j = decltype(J)::value;
        x0 = rec_ld(frs, rec_off(l > j, F::hv(j) + l - (j + 1)));
        x1 = rec_ld(frs, 8u * (unsigned)(F::hv(j) + J0 + l - (j + 1)));
      });
}

}  // namespace

}  // namespace cwbl
