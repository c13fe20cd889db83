// cwbl_tq_big_factor.hip — the factor cache's kernel pair of the hand-off path at KP = 96
// (k = 65..96, CWBL_OPT_BIG_REUSE):
//   fill_tqb_tail_kernel<KP, J0>     solve_tqb_tail_kernel<KP, J0, 2>'s analysis (cwbl_tq_tail.hip:
//                                    the same text, so the same bits) from the hand-off kernel's
//                                    record, which also leaves the point's factor as a
//                                    BigFactor<KP, J0> (cwbl_internal.h) with plain vector stores
//                                    that nothing waits for: its own pivot rows as each step forms
//                                    them, the hand-off kernel's reflectors as the back-transform
//                                    loads them, T, Q^T b1, tau and scal after the loop;
//   solve_tqb_factor_kernel<KP, J0>  the same analysis from that factor, one point per wavefront:
//                                    no lists, no assembly, no hand-off kernel, no record and no
//                                    dlarfg.  It replays the x' half of every step — steps j < J0
//                                    in the hand-off kernel's expressions and layout, steps
//                                    j >= J0 in the tail's — and then runs the quadrature, the
//                                    back-transform and the epilogue both kernels share
//                                    (tqb_finish).
// Shared with solve_tqb_tail_kernel through cwbl_tq_tail_common.h: the shared-memory struct
// (TailSmem), the point index and the fp32 readlane.  Both kept every kernel's instruction
// stream as it was (profiles/twin_merge.txt).  The two larger texts are still repeated, in
// cwbl_tq_big_factor.h (which the KP = 128 pair, cwbl_tq_rows_factor.hip, shares),
// because solve_tqb_tail_kernel, with either as a shared function, compiled to other vector
// code than with its own text (the numbers are in cwbl_tq_tail_common.h): the fill's hand-off
// load and Householder loop are the tail's with the factor's stores added, and tqb_finish is
// the tail's quadrature, back-transform and epilogue as a function over two row loaders.
#include "cwbl_tq_big_factor.h"

namespace cwbl {

// One point per wavefront from its BigFactor.  info[gi].x is the accepted count the fill left
// (restored by the host); the flags and alphas are this call's.
//
// Steps j < J0 are replayed as the hand-off kernel's waves 0 and 1 hold x': one register with
// row = lane, one with rows 64 .. KP-1 on lanes < KP - 64 and zeros elsewhere; v . x' is summed
// as its bsum4 sums it (a wave sum per wave, then (w0 + w1) + (w2 + w3), the two waves past KP
// adding zeros).  Steps j >= J0 run in the tail's layout (lane l is row J0 + l) and expressions.
// The loads are unconditional, each a constant offset from one lane offset into the point's own
// factor (a load under a lane mask is a branch of its own, and the waits behind such branches
// come out as vmcnt(0)); the row mask is applied at the use.  They are issued in the order of
// first use: the scalars and the J0 reflectors (two registers each) before step 0, two of the
// tail's columns behind each replayed step into the registers it released (all KP (KP - 1) / 2
// words at once do not fit the register file at two waves per SIMD), T and Q^T b1 last.
template <int KP, int J0>
__global__ void __launch_bounds__(64, 2)
solve_tqb_factor_kernel(SolveConsts c, SlabDev slab, long long g0, int npts,
                        const double *__restrict__ fac, int2 *__restrict__ info) {
  using F = BigFactor<KP, J0>;
  constexpr int KT = KP - J0;
  constexpr int NS = KT - 2;  // the tail's steps at k = KP
  static_assert(KT == 64 && KP > 64 && KP - 64 <= J0 && NS <= 2 * (J0 - 1),
                "rows 64 .. KP-1 on the prefix lanes; two tail columns behind each head step");
  using SM = TailSmem<KP, J0>;
  __shared__ SM sm;

  const int gi = xcd_remap_rev(blockIdx.x, gridDim.x);  // the tail's XCD-chunk order
  if (gi >= npts) return;
  const int l = threadIdx.x;
  const int k = c.k;
  const int ptot = info[gi].x;
  if (ptot == 0) return;  // no accepted observation: var and info stay as they are

  const long long P = bf_point_index(slab, g0 + gi);
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

  tqb_finish<KP, J0>(
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

hipError_t launch_fill_tqb_tail(hipStream_t s, int kp, SolveConsts c, SlabDev slab, long long g0,
                                int npts, double *ws, int2 *info, double *fac) {
  if (kp == 128) return launch_fill_tqb_tail_rows(s, c, slab, g0, npts, ws, info, fac);
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !ws || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((fill_tqb_tail_kernel<96, 32>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, ws, info, fac);
  return hipGetLastError();
}

hipError_t launch_solve_tqb_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   long long g0, int npts, const double *fac, int2 *info) {
  if (kp == 128) return launch_solve_tqb_factor_rows(s, c, slab, g0, npts, fac, info);
  if (npts <= 0) return hipSuccess;
  if (c.quad == nullptr || kp != 96 || c.k <= kp - 62 || !info || !fac)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((solve_tqb_factor_kernel<96, 32>), dim3(npts), dim3(64), 0, s, c, slab, g0,
                     npts, fac, info);
  return hipGetLastError();
}

}  // namespace cwbl
