// cwbl_tq_multi.hip — solve_tq_multi_kernel<KP, NV>: solve_tq_kernel<KP, false> (cwbl_tq.hip)
// for a group of variables that share a localisation (cwbl_analyze_vars) on the one-wavefront
// path: k <= 16, k = 41..64, and k = 17..40 under CWBL_OPT_SPLIT40 = 0.
//
// A = inflat I + Yb Yb^T, b1 = Yb d and therefore the factor A = Q T Q^T do not depend on the
// analysed variable; only x' does, and solve_tq_kernel's Householder step touches x' in three
// places: the product x . ux that rides in the step's four-value reduction, s2 and the ux
// update.  This kernel has solve_tq_kernel's layout (one point per wavefront, lane = member =
// row, the same shared-memory struct) and runs the staging, the MFMA assembly, b1, the trace,
// T and the reflectors once per point, carrying the x' of up to NV variables through the
// loop: ux[i] is one fp64 value per lane and variable, every x . ux[i] is formed in the
// step's reductions (wave_sum4_dpp adds its four slots by the same tree, so the slot a sum
// rides in does not change its bits), and s2_i and the ux[i] update are solve_tq_kernel's
// expressions.  The step's two early exits (j >= k - 2, tau == 0) are wave-uniform and skip
// every variable's update alike.  Slots past the group's nvar carry zeros.
//
// After the loop a run-time loop over the group's variables writes that variable's Q^T x'
// into the tq records and runs solve_tq_kernel's quadrature, d = u1 . T^-1 u2, back-transform
// and RTPP/RTPS epilogue with the variable's own flags and alphas, and stores its analysis.
// The variable's background is loaded again there (it is not kept across the loop: at KP = 64
// the registers are full).  Every expression is the one solve_tq_kernel evaluates (the
// project builds with -ffp-contract=off and the steps use explicit fma), so each variable's
// analysis equals solve_tq_kernel's bit for bit.
//
// NV is a compile-time class (2, 4, 8): register indices stay static.  The body repeats
// cwbl_tq.hip's text rather than sharing it, so that solve_tq_kernel compiles to what it was
// (DESIGN.md §3.1); shared through cwbl_tq_common.h are the shared-memory struct and the
// occupancy.
#include "cwbl_tq_common.h"

namespace cwbl {

static_assert(kTqMfmaAssembly, "solve_tq_multi_kernel is written for the MFMA assembly");

// Rows of Q^T x' kept in LDS instead of registers.  Only KP = 40 with eight variables needs
// any: its budget is 128 VGPRs (four waves per SIMD) and solve_tq_kernel<40> already fills
// it; four rows of 40 doubles take the LDS of a point from 9 536 to 10 816 B, 15 instead of
// 16 one-wave workgroups per CU.  (KP = 40 runs here only under CWBL_OPT_SPLIT40 = 0.)
template <int KP, int NV>
struct TqMultiLds {
  static constexpr int kRows = (KP == 40 && NV == 8) ? 4 : 0;
};

template <int KP, int NV>
__global__ void __launch_bounds__(64, TqOccupancy<KP>::kWaves)
solve_tq_multi_kernel(const TreeDesc *__restrict__ trees, SolveConsts c, SlabDev slab,
                      Tq40Vars vars, long long g0, int npts, const int *__restrict__ nbr_cnt,
                      const int *__restrict__ nbr_idx, int2 *__restrict__ info) {
  static_assert(KP % 8 == 0 && KP <= 64, "KP");
  static_assert(NV >= 2 && NV <= kMaxGroupVars, "NV");
  constexpr int H = KP / 2;
  constexpr int NBL = AsmLayout<KP>::NBL, NBLK = AsmLayout<KP>::NBLK;
  using SM = TqSmem<KP>;
  __shared__ SM sm;
  constexpr int NL = TqMultiLds<KP, NV>::kRows, NR = NV - NL;
  __shared__ double uxl[NL > 0 ? NL : 1][KP];  // (unused, and not allocated, where NL = 0)

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= npts) return;
  const int lane = threadIdx.x;
  const int k = c.k;
  const int nvar = vars.nvar;

  long long P;  // var index of member 0
  float3 pt = make_float3(0.0f, 0.0f, 0.0f);  // the point's projected x, y and altitude
  {
    const long long g = g0 + gi;
    const int i = (int)(g % slab.ix_lim);
    const long long r = g / slab.ix_lim;
    const int j = (int)(r % slab.iy_lim);
    const int kz = (int)(r / slab.iy_lim);
    P = i + (long long)slab.nx * (j + (long long)slab.ny * kz);
    slab_point(slab, g, pt.x, pt.y, pt.z);
  }
  // background of member `lane` in every variable of the group (0 in the slots past nvar)
  float xbl[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    xbl[i] = 0.0f;
    if (i < nvar && lane < k) xbl[i] = vars.var[i][P + slab.L * opaque_int(lane)];
  }

  int bi[NBL], bj[NBL];
  block_of_lane<KP>(lane, bi, bj);
  double acc[NBL][16];
  double b1acc;
  int ptot;
  {
    f64x4 tile[MfmaLayout<KP>::NTL];
    assemble_point_mfma<KP, kTqChunk, false>(sm.u.ch, trees, c, gi, lane, nbr_cnt, nbr_idx, pt,
                                             nullptr, nullptr, nullptr, tile, b1acc, ptot);
    if (ptot == 0) {  // no accepted observation: every var left unchanged (:220, :226)
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
  // xb_mean = sum(xb) * nmember_inv in fp32 (:671), sequential like the reference
  auto mean_of = [&](float xb) {
    float s = 0.0f;
    for (int mm = 0; mm < k; ++mm)
      s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xb), mm));
    return (double)(s * c.nmember_inv);
  };
  // x' of every variable, becomes Q^T x': slots 0 .. NR-1 in registers, the NL others (KP = 40
  // with eight variables only, where 128 VGPRs do not hold them) as rows of uxl; a row's
  // value on the lanes >= KP is 0 throughout (x and v vanish there) and is not stored
  double ux[NR];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double u = 0.0;
    if (i < nvar) {  // (wave-uniform)
      const double xb_mean = mean_of(xbl[i]);
      u = (lane < k) ? (double)xbl[i] - xb_mean : 0.0;
    }
    if (i < NR) ux[i] = u;
    else if (lane < KP) uxl[i - NR][lane] = u;
  }
  double ub = (lane < KP) ? b1acc : 0.0;  // Yb d, becomes Q^T b1

  // ---- Householder tridiagonalisation (lower, dsytd2 order) ------------------------------
  // solve_tq_kernel's steps (cwbl_tq.hip) with NV vectors ux in place of one.
  constexpr int J0T = SM::J0T, NB2 = SM::NB2, PLD2 = SM::PLD2;
  int bi2 = 0, bj2 = 0;  // this lane's block of the 2x2 phase (lane < NBLK2)
  while ((bi2 + 1) * (bi2 + 2) / 2 <= lane) ++bi2;
  bj2 = lane - bi2 * (bi2 + 1) / 2;
  const bool tail_lane = lane < SM::NBLK2;
  auto ld4 = [](const double *p, double (&o)[4]) {
    const double2 a0 = *reinterpret_cast<const double2 *>(p);
    const double2 a1 = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = a0.x; o[1] = a0.y; o[2] = a1.x; o[3] = a1.y;
  };
  auto step = [&](const int j, auto phase, auto q, double (&Ap)[NBL][16])
                  __attribute__((always_inline)) {
    constexpr bool ph2 = decltype(phase)::value;
    constexpr int qj = decltype(q)::value, q2 = qj;  // column within the block: constant
    double (&A)[NBL][16] = *[&]() {
      if constexpr (NBL == 1) return &acc; else return &Ap;
    }();
    const int J = j >> 2;
    const int J2 = (j - J0T) >> 1;
    if constexpr (ph2) {
      if (j == J0T) {  // re-deal the tail: 4x4 blocks -> packed lower triangle -> 2x2 blocks
        double *tri = &sm.u.reg[J0T < KP ? SM::pb2_base(0) : 0];
        constexpr int JB = J0T / 4;
#pragma unroll
        for (int it = 0; it < NBL; ++it) {
          if (lane + 64 * it < NBLK && bi[it] >= JB && bj[it] >= JB) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int a = 4 * (bi[it] - JB) + r, b = 4 * (bj[it] - JB) + q;
                if (a >= b) tri[a * (a + 1) / 2 + b] = A[it][4 * r + q];
              }
          }
        }
        __syncthreads();
        if (tail_lane) {
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const int a = 2 * bi2 + r, b = 2 * bj2 + q;
              A[0][2 * r + q] = a >= b ? tri[a * (a + 1) / 2 + b] : tri[b * (b + 1) / 2 + a];
            }
        }
        __syncthreads();
      }
    }
    if constexpr (!ph2) {
#pragma unroll
      for (int it = 0; it < NBL; ++it) {
        if (lane + 64 * it < NBLK && bj[it] == J) {  // publish column j
          *reinterpret_cast<double2 *>(&sm.col[4 * bi[it]]) =
              make_double2(A[it][qj], A[it][4 + qj]);
          *reinterpret_cast<double2 *>(&sm.col[4 * bi[it] + 2]) =
              make_double2(A[it][8 + qj], A[it][12 + qj]);
        }
      }
    } else if (tail_lane && bj2 == J2) {  // publish column j (2x2 phase)
      const double c0 = A[0][q2 & 1], c1 = A[0][2 + (q2 & 1)];
      *reinterpret_cast<double2 *>(&sm.col[J0T + 2 * bi2]) = make_double2(c0, c1);
    }
    __syncthreads();
    const double dj = sm.col[j];
    if (lane == 0) sm.tq[j][0] = dj;
    if (j >= k - 2) {  // trailing 2x2 block: already tridiagonal
      if (j == k - 2 && lane == 0) {
        sm.tq[j + 1][1] = sm.col[j + 1];
      }
      return;
    }
    const double x = (lane > j + 1 && lane < k) ? sm.col[lane] : 0.0;
    const double alpha = sm.col[j + 1];
    // x.x, x.ub and every x.ux[i], four per pass: v = x * scal + e_{j+1} gives
    // v.u = scal (x.u) + u_{j+1}.  The first pass is solve_tq_kernel's with variable 1 in the
    // pad slot.
    double xn2 = x * x, xub = x * ub, xux[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      xux[i] = x * (i < NR ? ux[i] : lane < KP ? uxl[i - NR][lane] : 0.0);
    wave_sum4_dpp(xn2, xux[0], xub, xux[1]);
#pragma unroll
    for (int i = 2; i < NV; i += 4) {
      if (i + 3 < NV) {
        wave_sum4_dpp(xux[i], xux[i + 1], xux[i + 2], xux[i + 3]);
      } else {
        double pad2 = 0.0, pad3 = 0.0;
        wave_sum4_dpp(xux[i], xux[i + 1], pad2, pad3);
      }
    }
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
    }
    if (tau == 0.0) return;  // H_j = I (uniform)
    // v_i = x_i * scal (i > j+1), v_{j+1} = 1, 0 elsewhere
    const double v = lane == j + 1 ? 1.0 : x * scal;
    if (lane < KP) sm.vb[lane] = v;
    if (lane > j && lane < k) sm.u.reg[SM::hv_off(0) + j * (k - 1) - j * (j - 1) / 2 + lane - (j + 1)] = v;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < NR) {
        const double s2 = fma(scal, xux[i], readlane_f64(ux[i], j + 1));  // v . ux
        ux[i] = fma(-tau * s2, v, ux[i]);
      } else {  // (row j + 1's value is the previous steps': barriers lie between)
        const double s2 = fma(scal, xux[i], uxl[i - NR][j + 1]);
        if (lane < KP) uxl[i - NR][lane] = fma(-tau * s2, v, uxl[i - NR][lane]);
      }
    }
    const double s3 = fma(scal, xub, readlane_f64(ub, j + 1));  // v . ub
    ub = fma(-tau * s3, v, ub);
    __syncthreads();
    // partials of A v (block rows >= J only: v vanishes above)
    double s1p = 0.0;  // this lane's share of v^T A v
    double pp = 0.0;
    if constexpr (!ph2) {
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
      s1p = s1;
    } else {
      double *pb = &sm.u.reg[SM::pb2_base(J2)] - J2 * PLD2;  // pb[R * PLD2 + col], R >= J2
      if (tail_lane && bi2 >= J2) {
        const double2 vi = *reinterpret_cast<const double2 *>(&sm.vb[J0T + 2 * bi2]);
        const double2 vj = *reinterpret_cast<const double2 *>(&sm.vb[J0T + 2 * bj2]);
        const double pr0 = fma(A[0][1], vj.y, A[0][0] * vj.x);
        const double pr1 = fma(A[0][3], vj.y, A[0][2] * vj.x);
        double sp = fma(vi.y, pr1, vi.x * pr0);
        *reinterpret_cast<double2 *>(pb + bi2 * PLD2 + 2 * bj2) = make_double2(pr0, pr1);
        if (bi2 != bj2) {
          if (bj2 >= J2) {
            const double pc0 = fma(A[0][2], vi.y, A[0][0] * vi.x);
            const double pc1 = fma(A[0][3], vi.y, A[0][1] * vi.x);
            *reinterpret_cast<double2 *>(pb + bj2 * PLD2 + 2 * bi2) = make_double2(pc0, pc1);
          }
          sp = sp + sp;
        }
        s1p = sp;
      }
      const double s1 = tau * wave_sum_dpp(s1p);
      __syncthreads();
      if (lane < KP && lane > j) {
        const double *prow = pb + ((lane - J0T) >> 1) * PLD2 + ((lane - J0T) & 1);
        pp = prow[0];
#pragma unroll
        for (int cb = 1; cb < NB2; ++cb) pp += prow[2 * cb];
      }
      s1p = s1;
    }
    const double s1 = s1p;
    const double p = (lane > j && lane < k) ? tau * pp : 0.0;
    const double w = fma(-0.5 * tau * s1, v, p);  // w = p - (tau/2)(p.v) v
    if (lane < KP) sm.wb[lane] = w;
    __syncthreads();
    // A <- A - v w^T - w v^T (rows and columns <= j are untouched: v, w vanish there)
    if constexpr (!ph2) {
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
    } else if (tail_lane && bi2 >= J2) {
      const double2 vi = *reinterpret_cast<const double2 *>(&sm.vb[J0T + 2 * bi2]);
      const double2 vj = *reinterpret_cast<const double2 *>(&sm.vb[J0T + 2 * bj2]);
      const double2 wi = *reinterpret_cast<const double2 *>(&sm.wb[J0T + 2 * bi2]);
      const double2 wj = *reinterpret_cast<const double2 *>(&sm.wb[J0T + 2 * bj2]);
      A[0][0] = fma(-vi.x, wj.x, fma(-wi.x, vj.x, A[0][0]));
      A[0][1] = fma(-vi.x, wj.y, fma(-wi.x, vj.y, A[0][1]));
      A[0][2] = fma(-vi.y, wj.x, fma(-wi.y, vj.x, A[0][2]));
      A[0][3] = fma(-vi.y, wj.y, fma(-wi.y, vj.y, A[0][3]));
    }
  };
  // unrolled by the block width, so that the pivot column's registers are known statically
  using std::false_type, std::true_type, std::integral_constant;
  const int jend1 = k < J0T ? k : J0T;
  for (int j = 0; j < jend1; j += 4) {
    step(j, false_type{}, integral_constant<int, 0>{}, acc);
    if (j + 1 < jend1) step(j + 1, false_type{}, integral_constant<int, 1>{}, acc);
    if (j + 2 < jend1) step(j + 2, false_type{}, integral_constant<int, 2>{}, acc);
    if (j + 3 < jend1) step(j + 3, false_type{}, integral_constant<int, 3>{}, acc);
  }
  if constexpr (J0T < KP) {
    static_assert(J0T % 2 == 0, "2x2 phase alignment");
    for (int j = J0T; j < k; j += 2) {
      step(j, true_type{}, integral_constant<int, 0>{}, acc);
      if (j + 1 < k) step(j + 1, true_type{}, integral_constant<int, 1>{}, acc);
    }
  }
  // after the Householder vectors (the partials are dead): per side, in walk order, the
  // quadrature sum (Ym) and node 31's exact solve (Zm)
  double *Ym = &sm.u.reg[SM::NHV], *Zm = Ym + KP;
  if (lane < KP) sm.tq[lane][2] = ub;
  __syncthreads();
  // trace of T (= trace of A) over the members in step order, as solve_tq_kernel's steps add
  // it, from the diagonal in LDS: no accumulator is live across the steps
  double trace = 0.0;
  for (int j = 0; j < k; ++j) trace += sm.tq[j][0];

  // ---- the quadrature rule of the point: T only, once ---------------------------------------
  // spectrum of A within [m, M]: m = inflat (A - inflat I = Yb Yb^T >= 0),
  // M = trace(A) - (k-1) m (the other k-1 eigenvalues are >= m)
  const double m = inflat_r8;
  const double ratio = trace / m - (double)(k - 1);
  int level = 1;
  double dec = 10.0;
  while (level < kQuadLevels && dec < ratio) {
    dec *= 10.0;
    ++level;
  }
  const int node = lane & 31, side = lane >> 5;
  const int npass = quad_passes(level);
  const double2 *rule = quad_rule(c.quad_r, npass == 1 ? 4 : 8, level);
  // byte offsets into sm.tq: row t of the walk at q0 + dirb t (opaque_after, cwbl_device.h)
  const unsigned q0 = side ? (KP - 1) * 32u : 0u, dirb = side ? (unsigned)-32 : 32u;
  const unsigned csb = side ? 40u : 8u;  // coupling with the previous mirrored row
  double *ym = Ym + side * H, *zm = Zm + side * H;
  const int wi = lane < H ? lane : H + (KP - 1 - lane);  // walk slot of row `lane`
  auto hvec = [&](int j) {
    const int off = j * (k - 1) - j * (j - 1) / 2;
    return (lane > j && lane < k) ? sm.u.reg[off + lane - (j + 1)] : 0.0;
  };
  // the reference's sequential sums run on wave-uniform values read lane by lane
  auto seq_sum = [&](float x) {
    float s = 0.0f;
    for (int mm = 0; mm < k; ++mm) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), mm));
    return s;
  };

  // ---- the variables of the group ----------------------------------------------------------
#pragma unroll 1
  for (int iv = 0; iv < nvar; ++iv) {
    float *__restrict__ const var = vars.var[iv];
    const int use_rtpp = vars.use_rtpp[iv], use_rtps = vars.use_rtps[iv];
    const float rtpp_alpha = vars.rtpp_alpha[iv], rtps_alpha = vars.rtps_alpha[iv];
    // the variable's Q^T x' (iv is wave-uniform: selects, not indexed registers)
    double uxi = ux[0];
#pragma unroll
    for (int i = 1; i < NR; ++i) uxi = iv == i ? ux[i] : uxi;
    if constexpr (NL > 0) {
      if (iv >= NR && lane < KP) uxi = uxl[iv - NR][lane];
    }
    if (lane < KP) sm.tq[lane][3] = uxi;
    // its background again, and xb_mean as before the loop
    float xb = 0.0f;
    // (the member offset is formed here, from an opaque lane index, not kept across the loop)
    const long long Pl = P + slab.L * opaque_int(lane);
    if (lane < k) xb = var[Pl];
    const double xb_mean = mean_of(xb);
    __syncthreads();

    // ---- T^-1/2 u2 by quadrature, u1^T T^-1 u2 exactly (solve_tq_kernel's passes) ---------
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
    const double zl = lane < KP ? Zm[wi] : 0.0;
    double yl = lane < KP ? Ym[wi] : 0.0;
    const double d = wave_sum_dpp(lane < KP ? sm.tq[lane][2] * zl : 0.0);  // u1 . T^-1 u2

    // ---- back-transform: y <- Q y = H_0 H_1 ... H_{k-3} y, two reflectors per reduction ---
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
    // (from an opaque k: formed here, not held in registers across the variable loop)
    const double sk = sqrt((double)(opaque_int(k) - 1));
    // analysis of member `lane` (xa = wbar, :675-679); fp32 from here on, in registers
    float xal = lane < KP ? (float)(xb_mean + (d + sk * yl)) : 0.0f;

    // ---- RTPP / RTPS (:684-698), fp32 in the reference's order, the variable's own flags --
    if (use_rtpp || use_rtps) {
      const float xa_mean = seq_sum(xal) * c.nmember_inv;
      const double xpl = lane < k ? (double)xb - xb_mean : 0.0;
      float xap = 0.0f;
      if (lane < k) {
        xap = xal - xa_mean;
        if (use_rtpp)
          xap = (float)((double)((1.0f - rtpp_alpha) * xap) + (double)rtpp_alpha * xpl);
      }
      if (use_rtps) {
        double d8 = 0.0;
        for (int mm = 0; mm < k; ++mm) {
          const double xp = readlane_f64(xpl, mm);
          d8 = d8 + xp * xp;
        }
        const float xb_std = (float)d8;
        const float xa_std = seq_sum(xap * xap);
        xap = xap * (rtps_alpha * sqrtf(xb_std / xa_std) - rtps_alpha + 1.0f);
      }
      xal = xa_mean + xap;
    }
    if (lane < k) var[P + slab.L * opaque_int(lane)] = xal;
    __syncthreads();  // the next variable rewrites tq[.][3], Ym and Zm
  }
  // info.y: decade of the quadrature rule (negative when M/m exceeds the last table); once
  if (lane == 0 && info) info[gi] = make_int2(ptot, ratio > dec ? -level : level);
}

template <int KP>
static hipError_t launch_tq_multi_kp(hipStream_t s, const TreeDesc *trees, SolveConsts c,
                                     SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                     const int *nbr_cnt, const int *nbr_idx, int2 *info) {
#define CWBL_TQM_LAUNCH(NV)                                                                     \
  hipLaunchKernelGGL((solve_tq_multi_kernel<KP, NV>), dim3(npts), dim3(64), 0, s, trees, c,     \
                     slab, vars, g0, npts, nbr_cnt, nbr_idx, info)
  switch (group_var_class(vars.nvar)) {
    case 2: CWBL_TQM_LAUNCH(2); break;
    case 4: CWBL_TQM_LAUNCH(4); break;
    default: CWBL_TQM_LAUNCH(8); break;
  }
#undef CWBL_TQM_LAUNCH
  return hipGetLastError();
}

hipError_t launch_solve_tq_multi(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                                 SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                 const int *nbr_cnt, const int *nbr_idx, int2 *info) {
  if (npts <= 0) return hipSuccess;
  if (c.quad_r == nullptr || vars.nvar < 2 || vars.nvar > kMaxGroupVars)
    return hipErrorInvalidValue;
#define CWBL_TQM_CASE(K)                                                                      \
  case K:                                                                                     \
    return launch_tq_multi_kp<K>(s, trees, c, slab, vars, g0, npts, nbr_cnt, nbr_idx, info);
  switch (kp) {
    CWBL_TQM_CASE(8)
    CWBL_TQM_CASE(16)
    CWBL_TQM_CASE(24)
    CWBL_TQM_CASE(32)
    CWBL_TQM_CASE(40)
    CWBL_TQM_CASE(48)
    CWBL_TQM_CASE(56)
    CWBL_TQM_CASE(64)
    default:
      return hipErrorInvalidValue;
  }
#undef CWBL_TQM_CASE
}

}  // namespace cwbl
