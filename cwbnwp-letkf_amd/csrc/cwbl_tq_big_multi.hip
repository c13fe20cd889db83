// cwbl_tq_big_multi.hip — solve_tq_big_multi_kernel<96, 32, NV>: the hand-off instantiation
// solve_tq_big_kernel<96, false, 32> (cwbl_tq_big.hip) for a group of variables that share a
// localisation (cwbl_analyze_vars) at k = 65..96: the staging, the assembly of
// A = (k-1)/infl I + Yb Yb^T and b1 = Yb d and the first 32 Householder steps on 4x4 register
// blocks once per point, with the x' of up to NV variables carried through the steps.
//
// A, b1 and so the reflectors do not depend on the analysed variable.  A step of
// solve_tq_big_kernel touches x' in three places: the product v * ux that rides in the step's
// four-value block reduction (bsum4), and the update ux = fma(-tau s2, v, ux).  Here ux[i] is
// one fp64 value per thread and variable: variable 0 rides in the slot it has in
// solve_tq_big_kernel, variable 1 in the reduction's free fourth slot, the others four per
// further wave pass, and the exchange through LDS is wide enough that the step keeps its one
// barrier there (wave_sum4_dpp adds its four slots by the same tree and the cross-wave sum is
// one expression per slot, so the slot a sum rides in does not change its bits).  Every
// variable's background is loaded by the thread of its member and its fp32 member sum runs
// in the reference's order, wave after wave.  Slots past the group's nvar carry zeros.  Every
// expression is the one solve_tq_big_kernel evaluates, so each variable's Q^T x' equals its
// bit for bit; the record is BigHandoffMulti<96, 32, NV>.
//
// The body repeats cwbl_tq_big.hip's text (its KP = 96 slab-mode hand-off path only) rather
// than sharing it, so that solve_tq_big_kernel compiles to what it was.
#include "cwbl_device.h"

#include <type_traits>

namespace cwbl {

namespace {

constexpr int kBigMThreads = 256;
constexpr int kBigMChunk = 32;  // columns staged per chunk (solve_tq_big_kernel's hand-off path)
constexpr int kBigMWaves = 3;   // waves per SIMD the register budget is sized for (168 VGPRs)

// thread -> 4x4 blocks of the lower block triangle: solve_tq_big_kernel's plan
// (big_block_of_lane, cwbl_tq_big.hip)
template <int KP>
__device__ __forceinline__ void bigm_block_of_lane(int tid, int (&bi)[AsmLayout<KP, 256>::NBL],
                                                   int (&bj)[AsmLayout<KP, 256>::NBL]) {
  using L = AsmLayout<KP, 256>;
  constexpr int NB = L::NB, NBL = L::NBL, F = 4 * (NBL - 1);
  constexpr int R = L::NBLK - 256 * (NBL - 1);  // blocks in the partial slots
  static_assert(NBL >= 1 && NBL <= 3 && R > 0, "slot plan");
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int it = 0; it < NBL; ++it) {
    int s;  // full-slot rank by lifetime
    if (it == 0) s = F - 1 - wave;
    else if (it == 1) s = wave;
    else s = F - 5 - wave;
    int b = it == NBL - 1 ? 64 * wave + lane : R + 64 * s + lane;
    if (b >= L::NBLK) b = L::NBLK - 1;  // invalid lane of a partial slot (never used)
    int cj = 0;
    while (b >= NB - cj) {  // column cj holds blocks bi = cj .. NB-1
      b -= NB - cj;
      ++cj;
    }
    bj[it] = cj;
    bi[it] = cj + b;
  }
}

// last block column of the partial slot NBL - 1 (blocks 0 .. R-1 in column-major order)
template <int KP>
constexpr int bigm_partial_last_column() {
  using L = AsmLayout<KP, 256>;
  int b = L::NBLK - 256 * (L::NBL - 1) - 1, cj = 0;
  while (b >= L::NB - cj) {
    b -= L::NB - cj;
    ++cj;
  }
  return cj;
}
static_assert(bigm_partial_last_column<96>() == 1, "JP");

// Slots of Q^T x' held in registers; the others live in LDS (BigMultiSmem::uxl).
// solve_tq_big_kernel<96, false, 32> sits in the 168 VGPRs of three waves per SIMD, which hold
// two more vectors beside it, not four.
constexpr int bigm_regs(int nv) { return nv < 2 ? nv : 2; }

}  // namespace

// (solve_tq_big_kernel's BigSmem without what only its one-kernel form uses, the block
// reductions' exchange widened to two values and NV variables)
template <int KP, int CHK, int NV>
struct BigMultiSmem {
  static constexpr int NB = KP / 4;
  static constexpr int PLD = 4 * NB + 4;  // 2*PLD = 8*odd dwords: conflict-free row sums
  union {
    ColumnChunk<KP, CHK, float, KP, false, KP == 128> ch[2];  // staged columns
    double pb[NB][PLD];                   // A v partials: pb[R][4c+r] = block (R,c), row r
  } u;
  double col[KP];                         // pivot column
  double vb[KP], wb[KP];                  // v and w of the current step; Yb d before
  double tq[KP + 1][4];                   // d_i, c(i-1,i) (the other two entries unused)
  double tau[KP];
  double red[2][4][2 + NV];               // [buffer][wave][value] of the block reductions
  // Q^T x' of the variables past the NR held in registers (thread t < KP: its own entry)
  double uxl[NV - bigm_regs(NV) > 0 ? NV - bigm_regs(NV) : 1][KP];
  float parf[NV];                         // sequential-sum partials handed wave to wave
  int ptot;
};

template <int KP, int HS, int NV>
__global__ void __launch_bounds__(kBigMThreads, kBigMWaves)
solve_tq_big_multi_kernel(const TreeDesc *__restrict__ trees, SolveConsts c, SlabDev slab,
                          Tq40Vars vars, long long g0, int npts,
                          const int *__restrict__ nbr_cnt, const int *__restrict__ nbr_idx,
                          int2 *__restrict__ info, double *__restrict__ ws) {
  static_assert(KP == 96 && HS == 32, "one instantiation: 96 rows, 32 steps");
  static_assert(NV >= 2 && NV <= kMaxGroupVars, "NV");
  constexpr int NT = kBigMThreads;
  using L = AsmLayout<KP, NT>;
  constexpr int NBL = L::NBL, NBLK = L::NBLK;
  constexpr int CHK = kBigMChunk;
  constexpr int NR = bigm_regs(NV);
  using SM = BigMultiSmem<KP, CHK, NV>;
  using HO = BigHandoffMulti<KP, HS, NV>;
  __shared__ SM sm;

  const int gi = xcd_remap(blockIdx.x, gridDim.x);
  if (gi >= npts) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = c.k;
  const int nvar = vars.nvar;

  int rbuf = 0;

  long long P = 0;
  float3 pt = make_float3(0.0f, 0.0f, 0.0f);
  {
    const long long g = g0 + gi;
    const int i = (int)(g % slab.ix_lim);
    const long long r = g / slab.ix_lim;
    const int j = (int)(r % slab.iy_lim);
    const int kz = (int)(r / slab.iy_lim);
    P = i + (long long)slab.nx * (j + (long long)slab.ny * kz);
    slab_point(slab, g, pt.x, pt.y, pt.z);
  }
  // background of member `tid` in every variable of the group (0 in the slots past nvar)
  float xbl[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    xbl[i] = 0.0f;
    if (i < nvar && tid < k) xbl[i] = vars.var[i][P + slab.L * tid];
  }

  int bi[NBL], bj[NBL];
  bigm_block_of_lane<KP>(tid, bi, bj);
  double acc[NBL][16];
  double b1acc;
  int ptot;
  assemble_point<KP, CHK, false, NT>(sm.u.ch[0], trees, c, gi, tid, nbr_cnt, nbr_idx, pt,
                                     nullptr, nullptr, nullptr, bi, bj, acc, b1acc, ptot);
  if (tid == 0) sm.ptot = ptot;  // counted by wave 0
  __syncthreads();
  ptot = sm.ptot;
  if (ptot == 0) {  // no accepted observation: every var left unchanged (:220, :226)
    if (tid == 0) info[gi] = make_int2(0, 0);
    return;
  }

  if (CWBL_DBG_STOP(c) == 1 || CWBL_DBG_STOP(c) >= 12) {  // timing ablation: assembly only
    double t = b1acc;
#pragma unroll
    for (int it = 0; it < NBL; ++it)
      if (tid + NT * it < NBLK) t += acc[it][0] + acc[it][15];
    if (tid == 0) info[gi] = make_int2(ptot, (int)t);
    return;
  }
  const double inflat_r8 = (double)c.inflat;
#pragma unroll
  for (int it = 0; it < NBL; ++it) {
    if (tid + NT * it < NBLK && bi[it] == bj[it]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 4 * bi[it] + r;
        acc[it][5 * r] = ii < k ? acc[it][5 * r] + inflat_r8 : 1.0;
      }
    }
  }
  if (tid < KP) {  // padding of T: decoupled unit rows
    sm.tq[tid][0] = 1.0;
    sm.tq[tid][1] = 0.0;
    sm.tau[tid] = 0.0;
  }
  if (tid == 0) sm.tq[KP][1] = 0.0;
  // the reference's sequential member-order sums (member m lives in thread m), wave by wave,
  // every variable's in one pass (fp32, :671)
  for (int w = 0; 64 * w < k; ++w) {
    if (wave == w) {
      const int n = min(64, k - 64 * w);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (i < nvar) {  // (uniform)
          float s = w == 0 ? 0.0f : sm.parf[i];
          for (int m = 0; m < n; ++m)
            s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xbl[i]), m));
          if (lane == 0) sm.parf[i] = s;
        }
      }
    }
    __syncthreads();
  }
  // x', then Q^T x': slots 0 .. NR-1 in registers, the others in uxl (a thread reads and
  // writes only its own entry there; the threads >= KP hold the 0.0 that stays 0.0)
  double ux[NR];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double u = 0.0;
    if (i < nvar) {
      const double xb_mean = (double)(sm.parf[i] * c.nmember_inv);
      u = (tid < k) ? (double)xbl[i] - xb_mean : 0.0;
    }
    if (i < NR) ux[i < NR ? i : 0] = u;
    else if (tid < KP) sm.uxl[i - NR][tid] = u;
  }
  auto uxv = [&](int i) {
    return i < NR ? ux[i < NR ? i : 0] : tid < KP ? sm.uxl[i - NR][tid] : 0.0;
  };
  double ub = (tid < KP) ? b1acc : 0.0;  // Yb d, then Q^T b1

  // (the step's 4-value groups in LDS keep their two halves swapped when bit 3 of the group
  // index is set: see solve_tq_big_kernel)
  auto hsw = [](int x) { return (x >> 3) & 1; };
  auto ld4s = [](const double *p, int sw, double (&o)[4]) {  // logical half 0 at p + 2 sw
    const double2 a0 = *reinterpret_cast<const double2 *>(p + 2 * sw);
    const double2 a1 = *reinterpret_cast<const double2 *>(p + 2 - 2 * sw);
    o[0] = a0.x; o[1] = a0.y; o[2] = a1.x; o[3] = a1.y;
  };
  auto st4s = [](double *p, int sw, double a0, double a1, double a2, double a3) {
    *reinterpret_cast<double2 *>(p + 2 * sw) = make_double2(a0, a1);
    *reinterpret_cast<double2 *>(p + 2 - 2 * sw) = make_double2(a2, a3);
  };
  const int tsw = tid ^ (hsw(tid >> 2) << 1);  // this thread's element of v and w
  auto pub4 = [](double *d, double a0, double a1, double a2, double a3) {
    *reinterpret_cast<double2 *>(d) = make_double2(a0, a1);
    *reinterpret_cast<double2 *>(d + 2) = make_double2(a2, a3);
  };
  // (QJ: the column within the block, static: the steps run four to a block column)
  auto publish = [&](int J_, auto QJ, auto NS, const int (&bI)[NBL], const int (&bJ)[NBL],
                     double *dst) {
    constexpr int q_ = decltype(QJ)::value;
#pragma unroll
    for (int it = 0; it < decltype(NS)::value; ++it) {
      if (tid + NT * it < NBLK && bJ[it] == J_) {
        const double *a_ = acc[it];
        pub4(&dst[4 * bI[it]], a_[q_], a_[4 + q_], a_[8 + q_], a_[12 + q_]);
      }
    }
  };

  // ---- Householder tridiagonalisation: the first HS steps (k > HS + 2: all full steps) -----
  const int jend = CWBL_DBG_STEPS(c) > 0 ? min(HS, CWBL_DBG_STEPS(c)) : HS;  // (ablation)
  auto step = [&](const int j, auto QJ, auto NS) {
    constexpr int ns = decltype(NS)::value;
    int bI[NBL], bJ[NBL];
#pragma unroll
    for (int it = 0; it < NBL; ++it) {
      bI[it] = opaque_int(bi[it]);
      bJ[it] = opaque_int(bj[it]);
    }
    constexpr int qj = decltype(QJ)::value;
    const int J = j >> 2;
    publish(J, QJ, NS, bI, bJ, sm.col);
    // x.x (x = column j below row j + 1) from the owners' registers, reduced with the publish
    // barrier.  Rows >= k hold exact zeros in columns < k, so no row bound is needed.
    {
      double xs = 0.0;
#pragma unroll
      for (int it = 0; it < ns; ++it) {
        if (tid + NT * it < NBLK && bJ[it] == J) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {  // row 4 bI + r > j + 1
            const bool below = bI[it] > J + 1 || (bI[it] == J ? r > qj + 1 : r > qj - 3);
            const double a = acc[it][4 * r + qj];
            xs = below ? fma(a, a, xs) : xs;
          }
        }
      }
      xs = wave_sum_dpp(xs);
      if (lane == 0) sm.red[rbuf][wave][0] = xs;
    }
    __syncthreads();
    const double xn2 = (sm.red[rbuf][0][0] + sm.red[rbuf][1][0]) +
                       (sm.red[rbuf][2][0] + sm.red[rbuf][3][0]);
    rbuf ^= 1;
    const double dj = sm.col[j];
    if (tid == 0) sm.tq[j][0] = dj;
    const double x = (tid > j + 1 && tid < k) ? sm.col[tid] : 0.0;
    const double alpha = sm.col[j + 1];
    double tau = 0.0, beta = alpha, scal = 0.0;
    if (xn2 > 0.0) {  // dlarfg, fp64 rcp/rsq refined to ~1 ulp
      const double a2 = fma(alpha, alpha, xn2);
      const double r = rsq64(a2);             // 1/|beta|
      beta = -copysign(a2 * r, alpha);
      tau = (beta - alpha) * -copysign(r, alpha);  // (beta - alpha) / beta
      scal = rcp64(alpha - beta);
    }
    if (tid == 0) {
      sm.tq[j + 1][1] = beta;
      sm.tau[j] = tau;
    }
    // tau = 0 (H_j = I) runs the step too, as an exact no-op (see solve_tq_big_kernel)
    const double v = tid == j + 1 ? 1.0 : x * scal;
    if (tid < KP) sm.vb[tsw] = v;
    __syncthreads();
    double s1p = 0.0;
#pragma unroll
    for (int it = 0; it < ns; ++it) {
      if (tid + NT * it < NBLK && bJ[it] >= J) {
        double vi[4], vj[4];
        ld4s(&sm.vb[4 * bI[it]], hsw(bI[it]), vi);
        ld4s(&sm.vb[4 * bJ[it]], hsw(bJ[it]), vj);
        double pr[4], pc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pr[r] = acc[it][4 * r] * vj[0];
#pragma unroll
          for (int q = 1; q < 4; ++q) pr[r] = fma(acc[it][4 * r + q], vj[q], pr[r]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          pc[q] = acc[it][q] * vi[0];
#pragma unroll
          for (int r = 1; r < 4; ++r) pc[q] = fma(acc[it][4 * r + q], vi[r], pc[q]);
        }
        double sp = vi[0] * pr[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) sp = fma(vi[r], pr[r], sp);
        st4s(&sm.u.pb[bI[it]][4 * bJ[it]], hsw(bI[it]), pr[0], pr[1], pr[2], pr[3]);
        if (bI[it] != bJ[it]) {
          if (bJ[it] >= J)
            st4s(&sm.u.pb[bJ[it]][4 * bI[it]], hsw(bJ[it]), pc[0], pc[1], pc[2], pc[3]);
          sp = sp + sp;
        }
        s1p += sp;
      }
    }
    // v.A v, v.b1 and every v.x' in one block reduction (its barrier also publishes pb):
    // variable 0 in solve_tq_big_kernel's slot, variable 1 in its free fourth slot, the others
    // four per wave pass
    double s3 = v * ub;
    {
      double(*r)[2 + NV] = sm.red[rbuf];
      rbuf ^= 1;
      double a0 = v * uxv(0), a1 = v * uxv(1);
      wave_sum4_dpp(s1p, a0, s3, a1);
      if (lane == 0) {
        r[wave][0] = s1p;
        r[wave][1] = s3;
        r[wave][2] = a0;
        r[wave][3] = a1;
      }
#pragma unroll
      for (int i = 2; i < NV; i += 4) {
        double b0 = v * uxv(i), b1 = v * uxv(i + 1), b2 = 0.0, b3 = 0.0;
        if (i + 3 < NV) {
          b2 = v * uxv(i + 2);
          b3 = v * uxv(i + 3);
        }
        wave_sum4_dpp(b0, b1, b2, b3);
        if (lane == 0) {
          r[wave][2 + i] = b0;
          r[wave][3 + i] = b1;
          if (i + 3 < NV) {
            r[wave][4 + i] = b2;
            r[wave][5 + i] = b3;
          }
        }
      }
      __syncthreads();
      s1p = (r[0][0] + r[1][0]) + (r[2][0] + r[3][0]);
      s3 = (r[0][1] + r[1][1]) + (r[2][1] + r[3][1]);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const double s2 = (r[0][2 + i] + r[1][2 + i]) + (r[2][2 + i] + r[3][2 + i]);
        if (i < NR) ux[i < NR ? i : 0] = fma(-tau * s2, v, ux[i < NR ? i : 0]);
        else if (tid < KP) sm.uxl[i - NR][tid] = fma(-tau * s2, v, sm.uxl[i - NR][tid]);
      }
    }
    ub = fma(-tau * s3, v, ub);
    const double s1 = s1p * tau;  // p . v with p = tau A v
    double pp = 0.0;
    if (tid < KP && tid > j) {
      const double *prow = &sm.u.pb[tid >> 2][tsw & 3];
      // block columns < J hold exact zeros (dead blocks): start at the 8-column segment of J
      auto rsum = [&](auto C) {
        constexpr int c0 = decltype(C)::value;
        double t = 0.0;
#pragma unroll
        for (int cb = c0; cb < SM::NB; ++cb) t += prow[4 * cb];
        return t;
      };
      const int seg = J >> 3;
      if (seg >= 3 && SM::NB > 24) pp = rsum(std::integral_constant<int, (SM::NB > 24 ? 24 : 0)>{});
      else if (seg >= 2) pp = rsum(std::integral_constant<int, 16>{});
      else if (seg >= 1) pp = rsum(std::integral_constant<int, 8>{});
      else pp = rsum(std::integral_constant<int, 0>{});
    }
    const double p = (tid > j && tid < k) ? tau * pp : 0.0;
    const double w = fma(-0.5 * tau * s1, v, p);
    if (tid < KP) sm.wb[tsw] = w;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ns; ++it) {
      if (tid + NT * it < NBLK && bJ[it] >= J) {
        double vi[4], vj[4], wi[4], wj[4];
        ld4s(&sm.vb[4 * bI[it]], hsw(bI[it]), vi);
        ld4s(&sm.vb[4 * bJ[it]], hsw(bJ[it]), vj);
        ld4s(&sm.wb[4 * bI[it]], hsw(bI[it]), wi);
        ld4s(&sm.wb[4 * bJ[it]], hsw(bJ[it]), wj);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[it][4 * r + q] = fma(-vi[r], wj[q], fma(-wi[r], vj[q], acc[it][4 * r + q]));
        if (bJ[it] == J) {  // keep v_j in the entries of column j the steps no longer read
          const int r0 = j + 2 - 4 * bI[it];  // rows r >= r0 of the block
          auto keep = [&](auto Q) {
            constexpr int q = decltype(Q)::value;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[it][4 * r + q] = r >= r0 ? vi[r] : acc[it][4 * r + q];
          };
          keep(QJ);
        }
      }
    }
  };
  auto block_column = [&](int j0, auto NS) {  // four steps per block column: qj static
    step(j0, std::integral_constant<int, 0>{}, NS);
    if (j0 + 1 < jend) step(j0 + 1, std::integral_constant<int, 1>{}, NS);
    if (j0 + 2 < jend) step(j0 + 2, std::integral_constant<int, 2>{}, NS);
    if (j0 + 3 < jend) step(j0 + 3, std::integral_constant<int, 3>{}, NS);
  };
  // hand-off of slot it's blocks: trailing blocks as the full matrix, the others as reflector
  // columns
  double *__restrict__ wo = ws + (long long)gi * HO::WORDS;
  auto handoff_slot = [&](auto IT) {
    constexpr int it = decltype(IT)::value;
    constexpr int KT = HO::KT, JB = HS / 4;
    if (tid + NT * it < NBLK) {
      if (bj[it] >= JB) {  // trailing block: both triangles of the full KT x KT matrix
        const int a0 = 4 * (bi[it] - JB), b0 = 4 * (bj[it] - JB);
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // column b0 + q, rows a0 .. a0 + 3
          double *d = wo + HO::TA + (b0 + q) * KT + a0;
          pub4(d, acc[it][q], acc[it][4 + q], acc[it][8 + q], acc[it][12 + q]);
        }
        if (bi[it] != bj[it]) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {  // column a0 + r, rows b0 .. b0 + 3
            double *d = wo + HO::TA + (a0 + r) * KT + b0;
            pub4(d, acc[it][4 * r], acc[it][4 * r + 1], acc[it][4 * r + 2], acc[it][4 * r + 3]);
          }
        }
      } else {  // reflector columns j = 4 bj + q: v_j at rows > j (1 at row j + 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = 4 * bj[it] + q, a0 = 4 * bi[it];
          double e[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = a0 + r;
            e[r] = a == j + 1 ? 1.0 : a > j + 1 ? acc[it][4 * r + q] : 0.0;
          }
          pub4(wo + HO::HV + j * KP + a0, e[0], e[1], e[2], e[3]);
        }
      }
    }
  };
  constexpr int JP = bigm_partial_last_column<KP>();
  static_assert(JP < HS / 4, "the partial slot holds reflector columns only");
  int j0 = 0;
  for (; j0 < jend && j0 < 4 * (JP + 1); j0 += 4) block_column(j0, std::integral_constant<int, NBL>{});
  // the partial slot's blocks (reflector columns <= JP) go out now, so that its registers are
  // free for the remaining steps
  handoff_slot(std::integral_constant<int, NBL - 1>{});
  for (; j0 < jend; j0 += 4) block_column(j0, std::integral_constant<int, NBL - 1>{});
  __syncthreads();  // T, tau of the last steps are in LDS
  sfor<NBL - 1>([&](auto IT) { handoff_slot(IT); });
  if (tid < KP) {
    wo[HO::U1 + tid] = ub;
#pragma unroll
    for (int i = 0; i < NV; ++i) wo[HO::u2(i) + tid] = uxv(i);
  }
  if (tid < HS) {
    wo[HO::D + tid] = sm.tq[tid][0];
    wo[HO::E + tid] = sm.tq[tid + 1][1];
    wo[HO::TAU + tid] = sm.tau[tid];
  }
  if (tid == 0) info[gi] = make_int2(ptot, 0);
}

hipError_t launch_big_handoff_multi(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                                    SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                    const int *nbr_cnt, const int *nbr_idx, int2 *info,
                                    double *ws) {
  if (npts <= 0) return hipSuccess;
  if ((kp != 96 && kp != 128) || c.k <= kp - 62 || vars.nvar < 2 || vars.nvar > kMaxGroupVars)
    return hipErrorInvalidValue;
  // KP = 128 runs the half-row kernel (cwbl_tq_rows_multi.hip), as launch_big_handoff does
  if (kp == 128)
    return launch_rows_handoff_multi(s, trees, c, slab, vars, g0, npts, nbr_cnt, nbr_idx, info,
                                     ws);
#define CWBL_BIGM_LAUNCH(NV)                                                                    \
  hipLaunchKernelGGL((solve_tq_big_multi_kernel<96, 32, NV>), dim3(npts), dim3(kBigMThreads), 0, \
                     s, trees, c, slab, vars, g0, npts, nbr_cnt, nbr_idx, info, ws)
  switch (group_var_class(vars.nvar)) {
    case 2: CWBL_BIGM_LAUNCH(2); break;
    case 4: CWBL_BIGM_LAUNCH(4); break;
    default: CWBL_BIGM_LAUNCH(8); break;
  }
#undef CWBL_BIGM_LAUNCH
  return hipGetLastError();
}

}  // namespace cwbl
