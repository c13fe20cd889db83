// cwbl_tq_tail_common.h — what the kernels that finish the hand-off path's solve (k = 65..128,
// one grid point per wavefront, lane l holding the full trailing row J0 + l) share:
// solve_tqb_tail_kernel (cwbl_tq_tail.hip), fill_tqb_tail_kernel and solve_tqb_factor_kernel
// (cwbl_tq_big_factor.h, instantiated by cwbl_tq_big_factor.hip at KP = 96 and by
// cwbl_tq_rows_factor.hip at KP = 128) and solve_tqb_tail_multi_kernel (cwbl_tq_tail_multi.hip).
//
// Only the shared-memory struct and the fp32 readlane: with them every kernel's instruction
// stream is what it was.  The texts these kernels repeat stay twins, because as functions
// inlined into their kernels they compile to other code than in the kernels' own bodies
// (profiles/twin_merge.txt has the numbers; a fix lands in every file that has the region):
//   var index of the point                          tail = tail_multi = bf_point_index
//       (cwbl_tq_big_factor.h); as one function it moves three instructions of the tail's
//       and the group kernels' prologue, which alone would ask for a timing run of eight
//       kernels
//   hand-off load and Householder steps J0 .. k-3   tail = fill (which adds the factor's
//                                                   stores); tail_multi carries NV vectors
//       as one function with a sink for the stores, the unroller leaves one more copy of a
//       step of the block of columns 48..55 in solve_tqb_tail_kernel (48 v_fmac_f64_dpp and
//       the step's swaps, rcp and rsq more at both KP; registers and scratch unchanged)
//   quadrature, back-transform, epilogue            tail = tail_multi (in its variable loop)
//                                                   = tqb_finish (cwbl_tq_big_factor.h: the
//                                                   fill and the factor kernels, one text)
//       through tqb_finish the backward sweep's segment loop is unrolled further:
//       solve_tqb_tail_kernel<96, 32, 2> takes 199 VGPRs for 193, <128, 64, 3> 116 B of
//       scratch for 140, the six group kernels 4 to 6 VGPRs more each
#pragma once

#include "cwbl_device.h"

namespace cwbl {

__device__ __forceinline__ float readlane_f32(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

template <int KP, int J0>
struct TailSmem {
  static constexpr int KT = KP - J0;
  double row[KT];         // a row of the trailing 2x2 block's step
  double tq[KP + 1][4];   // d_i, c(i-1,i), (Q^T b1)_i, (Q^T x')_i
  double tau[KP];
  double scl[KP];         // the tail's reflectors: v = scl * x below row j + 1
  double Ym[KP], Zm[KP];  // quadrature sum / exact solve, walk order
};

}  // namespace cwbl
