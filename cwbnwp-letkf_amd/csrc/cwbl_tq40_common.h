// cwbl_tq40_common.h — what solve_tq40_kernel (cwbl_tq40.hip) and tq40_passes
// (cwbl_tq40_passes.h: the one body of solve_tq40_multi_kernel, over the variables of a group,
// and of solve_tq40_column_kernel, over the levels of a column) share: the layout (four points
// per wavefront, one 16-lane DPP row per point; lane l holds the full rows J0 + l + 16 r of A
// in registers and, for l < J0, row l of the top-left J0 x J0 prefix block), the row sums, the
// shared-memory struct, dlarfg, the point decode, the record load, the trace and the wave's
// quadrature rounds.  Every function is inlined into its kernel; the kernels evaluate the
// same expressions in the same order, so a variable's analysis is the same bit pattern from
// any of them.  The tridiagonalisations (and the passes' replay) are the texts' own.  So are,
// as the same text in both, the quadrature's level and round loops and the RTPP/RTPS
// epilogue: each piece here was kept only where the kernels compiled to the registers, LDS
// and instruction mix they had without it and ran as fast.
//
// The twin regions, for whoever changes the numerics (a fix lands in every text that has the
// region; `single` = cwbl_tq40.hip; `passes` = cwbl_tq40_passes.h, one text for the group and
// the column kernel, which differ in its passes policy only; `fill` and `factor` =
// fill_tq40_factor_kernel and solve_tq40_factor_kernel in cwbl_tq40_fill.hip, which share one
// text, tq40_factor_solve, for everything after the factor: the passes' loop body at one
// variable, with Q^T b1, the accepted count and the var index re-read or recomputed at their
// uses):
//   phase 1 and phase 2 of the tridiagonalisation   single (carries x' too, keeps x scal);
//                                                   passes = fill (b1 only, keep x and scal;
//                                                   fill stores them with beta and tau, factor
//                                                   loads them: no step of its own)
//   quadrature level loop and LDS walk offsets      single = passes = fill/factor
//   replay of the reflectors on x'                  passes = fill/factor
//   quadrature round loop and d                     single = passes = fill/factor
//   back-transform                                  single (from x scal);
//                                                   passes = fill/factor
//   RTPP / RTPS epilogue and the store              single = passes = fill/factor
#pragma once

#include "cwbl_device.h"

namespace cwbl {

// Rank-2 updates run in groups of kUG columns, each group's first products before its second
// ones, so no fused FMA reads the accumulator the one before it wrote (the compiler puts an
// s_nop between two inline-asm statements that share a register); the matvec keeps kNA
// partial sums per row (column c -> sum c % kNA).  r6 A/B of the alternatives:
// profiles/r6_tq40_ab.txt.
constexpr int kUG = 8;
constexpr int kNA = 2;
template <int NS>
__device__ __forceinline__ double acc_sum(const double (&pa)[kNA][NS], int r) {
  return pa[0][r] + pa[1][r];
}

template <int KP>
struct Tq40Layout {
  static constexpr int J0 = kTq40J0;  // steps with the prefix block (phase 1)
  static constexpr int KT = KP - J0;  // slot rows J0 + l + 16 r
  static constexpr int NS = KT / 16;  // row slots per lane
  static constexpr int NV = NS + 1;   // vector slots: 0 = rows l < J0, 1.. = row slots
  static constexpr int H = KP / 2;    // rows walked by each side of a twisted solve
  static_assert(KT % 16 == 0 && J0 <= 16 && J0 >= 2 && KP % 2 == 0, "tq40 layout");
};

template <int KP>
struct Tq40Smem {
  // phase 1's reflectors, column j by row (rows <= j + 1 unused; the multi kernel keeps other
  // words there, see its phase 1)
  double pv[4][kTq40J0][KP];
  double qs[4][KP];           // per quadrature round: sum over the round's nodes of omega x(row)
  double qz[4][KP + 1];       // T^-1 u2 (slot 7 of the last round); [KP]: other lanes' dump
  double tq[4][KP + 1][4];    // d_i, c(i-1,i), (Q^T b1)_i, (Q^T x')_i
  double tau[4][KP];
};

// Sum over this lane's 16-lane row, the same value on every lane: two quad_perm stages (two
// v_mov_b32_dpp and a v_add_f64 each: gfx950 has no 64-bit quad_perm), then the four quad
// sums Q0 + Q4 + Q8 + Q12 as one row_newbcast move and three fused v_fmac_f64_dpp (x 1.0,
// one rounding each, as an add): 10 VALU instructions instead of row16_sum's 12.  The quad
// sum is read by DPP two or more wait states after its add (the move's own hazard nop).
__device__ __forceinline__ double rsum16(double v) {
  v += dpp_f64<0xB1>(v);  // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);  // quad_perm [2,3,0,1]
  double s = rbcast<0>(v);
  s = fmac_row<4>(s, v, 1.0);
  s = fmac_row<8>(s, v, 1.0);
  return fmac_row<12>(s, v, 1.0);
}

// Three row sums, stage by stage: each stage's DPP reads come three instructions after the
// adds that feed them, so no wait states are needed between the stages (the same sums, the
// same rounding order as rsum16)
__device__ __forceinline__ void rsum16x3(double &a, double &b, double &c) {
  a += dpp_f64<0xB1>(a);
  b += dpp_f64<0xB1>(b);
  c += dpp_f64<0xB1>(c);
  a += dpp_f64<0x4E>(a);
  b += dpp_f64<0x4E>(b);
  c += dpp_f64<0x4E>(c);
  double sa = rbcast<0>(a), sb = rbcast<0>(b), sc = rbcast<0>(c);
  sa = fmac_row<4>(sa, a, 1.0);
  sb = fmac_row<4>(sb, b, 1.0);
  sc = fmac_row<4>(sc, c, 1.0);
  sa = fmac_row<8>(sa, a, 1.0);
  sb = fmac_row<8>(sb, b, 1.0);
  sc = fmac_row<8>(sc, c, 1.0);
  a = fmac_row<12>(sa, a, 1.0);
  b = fmac_row<12>(sb, b, 1.0);
  c = fmac_row<12>(sc, c, 1.0);
}

// N row sums stage by stage (rsum16x3's interleaving for the prefix rows' column sums; the
// same rounding order as rsum16)
template <int N>
__device__ __forceinline__ void rsum16xN(double (&a)[N]) {
  double s[N];
  sfor<N>([&](auto ii) { a[decltype(ii)::value] += dpp_f64<0xB1>(a[decltype(ii)::value]); });
  sfor<N>([&](auto ii) { a[decltype(ii)::value] += dpp_f64<0x4E>(a[decltype(ii)::value]); });
  sfor<N>([&](auto ii) { s[decltype(ii)::value] = rbcast<0>(a[decltype(ii)::value]); });
  sfor<N>([&](auto ii) {
    constexpr int i = decltype(ii)::value;
    s[i] = fmac_row<4>(s[i], a[i], 1.0);
  });
  sfor<N>([&](auto ii) {
    constexpr int i = decltype(ii)::value;
    s[i] = fmac_row<8>(s[i], a[i], 1.0);
  });
  sfor<N>([&](auto ii) {
    constexpr int i = decltype(ii)::value;
    a[i] = fmac_row<12>(s[i], a[i], 1.0);
  });
}

// dlarfg with fp64 rcp/rsq refined to ~1 ulp; H = I when x = 0 (tau = 0, v = e_j+1)
struct Refl {
  double beta, tau, scal;
};
__device__ __forceinline__ Refl dlarfg(double alpha, double xx) {
  const double a2 = fma(alpha, alpha, xx);
  const double rs = rsq64(a2);  // 1/|beta|
  const bool nz = xx > 0.0;
  const double bt = -copysign(a2 * rs, alpha);
  Refl h;
  h.beta = nz ? bt : alpha;
  h.tau = nz ? (bt - alpha) * -copysign(rs, alpha) : 0.0;
  const double rab = rcp64(alpha - bt);
  h.scal = nz ? rab : 0.0;
  return h;
}

// var index of member 0 of slab point g0 + gi (g = i + ix_lim (j + iy_lim kz); g < 2^32: var
// would exceed HBM first)
__device__ __forceinline__ long long tq40_var_index(const SlabDev &slab, long long g0, int gi) {
  const unsigned g = (unsigned)(g0 + gi);
  const unsigned ix = (unsigned)slab.ix_lim, iy = (unsigned)slab.iy_lim;
  const unsigned rr = g / ix, ii = g - rr * ix, kz = rr / iy, jj = rr - kz * iy;
  return ii + (long long)slab.nx * (jj + (long long)slab.ny * kz);
}

// global row of lane l's vector slot vs (rows that do not exist get KP + 1: never < k)
template <int KP>
__device__ __forceinline__ int tq40_vrow(int l, int vs) {
  constexpr int J0 = kTq40J0;
  return vs == 0 ? (l < J0 ? l : KP + 1) : J0 + l + 16 * (vs - 1);
}

// fp32 sum over members in member order; member m is row m: prefix slot lane m (m < J0),
// else row slot (m - J0) / 16, lane (m - J0) % 16.  Every caller's x is +0 on the rows past
// k, and s + 0 = s (s is never -0), so the rows past k need no mask and each term is one
// v_add_f32 with a row_newbcast source.
template <int KP>
__device__ __forceinline__ float seq_sum_f32(const float (&x)[Tq40Layout<KP>::NV]) {
  constexpr int J0 = kTq40J0;
  float s = 0.0f;
  sfor<KP>([&](auto mm) {
    constexpr int m = decltype(mm)::value;
    constexpr int vs = m < J0 ? 0 : 1 + (m - J0) / 16, ln = m < J0 ? m : (m - J0) % 16;
    s = s + rbcast<ln>(x[vs]);
  });
  return s;
}

// A (slot rows, all columns), the prefix block row Pb (lanes >= J0 hold row 0's copy, never
// used) and b1 (ubP on the prefix rows, 0 on the lanes >= J0; ub on the slot rows) of point
// gi = 4 g4 + q from its record.
// A(t, col) of row t = J0 + l + 16 r: packed word tri(t) + col where col <= t, tri(col) + t
// above.  A column at or left of the slot's first row is in the lower part on every lane, one
// right of its last row in the upper part: one lane base plus a compile-time offset each,
// and only the columns inside the slot's row range pick per lane.  The loads go through a
// buffer resource on the wave's four records (a lane past the batch reads the spare record
// npts, at most three records on: the host allocates npts + 1), so the compile-time part of
// each offset sits in the instruction's offset fields instead of a per-load address
// computation.  (r6, measured and dropped: staging the records through LDS with coalesced
// 16-byte loads — equal at best, the per-lane gathers cost latency, not address throughput.)
template <int KP>
__device__ __forceinline__ void tq40_load_record(const double *__restrict__ ws, int g4, int q,
                                                 int l, bool valid, int npts,
                                                 double (&A)[Tq40Layout<KP>::NS][KP],
                                                 double (&Pb)[kTq40J0], double &ubP,
                                                 double (&ub)[Tq40Layout<KP>::NS]) {
  using HO = AsmRecord<KP>;
  constexpr int J0 = kTq40J0, NS = Tq40Layout<KP>::NS;
  const int gi = 4 * g4 + q;
  const int lp = l < J0 ? l : 0;
  // record words of this point: SGPR base + 32-bit offset (the host keeps a batch's records
  // below 2^32 bytes)
  const unsigned wb = (unsigned)(valid ? gi : npts) * (unsigned)HO::WORDS;
  auto w = [&](int i) { return gld(ws, wb + (unsigned)i); };
  const __amdgpu_buffer_rsrc_t rs = rec_rsrc(ws + (size_t)(4 * g4) * HO::WORDS, 4 * HO::WORDS);
  const unsigned rq = (unsigned)(valid ? q : npts - 4 * g4) * (unsigned)HO::WORDS;
  auto rw = [&](unsigned vword, unsigned cword) {  // record word vword + cword (cword static)
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(8u * vword), (int)(8u * cword), 0);
    return __longlong_as_double(((long long)v[1] << 32) | (unsigned)v[0]);
  };
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    constexpr int T0 = J0 + 16 * r, T1 = T0 + 15;  // the slot's rows
    const int t = T0 + l;
    const unsigned lo = rq + (unsigned)(HO::TA + t * (t + 1) / 2), up = rq + (unsigned)(HO::TA + t);
    sfor<KP>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      constexpr unsigned tc = (unsigned)(col * (col + 1) / 2);
      if constexpr (col <= T0) A[r][col] = rw(lo, col);
      else if constexpr (col > T1) A[r][col] = rw(up, tc);
      else A[r][col] = rw(col <= t ? lo + col : up + tc, 0u);
    });
  });
  {
    const unsigned lo = rq + (unsigned)(HO::TA + lp * (lp + 1) / 2), up = rq + (unsigned)(HO::TA + lp);
    sfor<J0>([&](auto cc) {
      constexpr int col = decltype(cc)::value;
      Pb[col] = rw(col <= lp ? lo + col : up + (unsigned)(col * (col + 1) / 2), 0u);
    });
  }
  {
    const double b = w(HO::U1 + lp);
    ubP = l < J0 ? b : 0.0;
  }
  sfor<NS>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int t = J0 + l + 16 * r;
    ub[r] = w(HO::U1 + t);
  });
}

// trace of T (= trace of A) over the members, from the diagonal in LDS: summed after the
// tridiagonalisation, not step by step, so that no step's d_j stays live to the end
template <int KP>
__device__ __forceinline__ double tq40_trace(const Tq40Smem<KP> &sm, int q, int l, int k) {
  double tp = 0.0;
  sfor<(KP + 15) / 16>([&](auto rr) {
    constexpr int r = decltype(rr)::value;
    const int i = l + 16 * r;
    if (16 * r + 15 < KP || i < KP) tp += i < k ? sm.tq[q][i < KP ? i : 0][0] : 0.0;
  });
  return rsum16(tp);
}

// Rounds of 8 quadrature nodes: the wave's largest need (quad_rounds) over its four points;
// each point then uses the (8 R - 1)-node rule of its own level.  (The level itself, a loop
// over the decades of M/m, stays in the kernels: moved here it compiles to other code.)
__device__ __forceinline__ int tq40_wave_rounds(int level) {
  const int rp = quad_rounds(level);
  return __ballot(rp == 8) ? 8 : __ballot(rp == 4) ? 4 : __ballot(rp == 3) ? 3 : 2;
}

}  // namespace cwbl
