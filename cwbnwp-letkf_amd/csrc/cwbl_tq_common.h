// cwbl_tq_common.h — what solve_tq_kernel (cwbl_tq.hip) and solve_tq_multi_kernel
// (cwbl_tq_multi.hip) share: the assembly mode, the shared-memory struct of one point and the
// occupancy the register allocation is held to.  The kernels' bodies are their own.
#pragma once

#include "cwbl_device.h"

#include <type_traits>

namespace cwbl {

// Assembly of Yb Yb^T: fp64 FMAs on the lower 4x4 blocks from columns staged in LDS as
// fp64 (16 per round), or on the matrix cores (v_mfma_f64_16x16x4 on 16x16 tiles of
// [Yb; yo], 32 float columns per round).  On gfx950 the FP64 matrix and vector rates are
// equal and the two do not co-issue; the tiles waste 44% of their products at KP = 40, so
// the block form is faster.  The MFMA form is kept for comparison (kTqMfmaAssembly).
constexpr bool kTqMfmaAssembly = true;
constexpr int kTqChunk = kTqMfmaAssembly ? 32 : 16;  // columns staged per round
using TqStage = std::conditional_t<kTqMfmaAssembly, float, double>;

// LDS of one point (KP = 40: 9.4 KB, so 16 waves fit a CU).  The big union is reused by
// phase: staged columns -> half of A -> {Householder vectors + A v partials}, then
// {Householder vectors + Q^T b1, Q^T x', T^-1/2 u2}.  The A v partials of step j only need
// block rows >= j/4 and sit at the top of the region, above the Householder vectors
// written so far.
template <int KP>
struct TqSmem {
  static constexpr int NB = KP / 4;
  static constexpr int PLD = 4 * NB + 4;  // pb row pitch: 2*PLD = 8*odd dwords, so the 8 block
                                          // rows of a half wave hit disjoint bank octets
  // Trailing phase: from step J0T on, the remaining kTail x kTail matrix is held as 2x2
  // blocks (NB2*(NB2+1)/2 = 55 <= 64 lanes), 4x fewer FMAs per lane than 4x4 blocks.
  static constexpr int kTail = 20;
  // (KP = 40 only: with more than one 4x4 block per lane the two phases' live ranges spill)
  static constexpr int J0T = KP == 40 ? KP - kTail : KP;  // first step of the 2x2 phase
  static constexpr int NB2 = kTail / 2;
  static constexpr int NBLK2 = NB2 * (NB2 + 1) / 2;
  static constexpr int PLD2 = 2 * NB2 + 2;  // 2x2-phase partials pitch (>= the packed tail)
  static_assert(NB2 * PLD2 >= kTail * (kTail + 1) / 2 && NBLK2 <= 64, "tail layout");
  static constexpr int NHV = KP * (KP - 1) / 2;  // packed Householder vectors at k = KP
  static constexpr int hv_off(int j) { return j * (KP - 1) - j * (j - 1) / 2; }
  static constexpr int cap() {  // region size: vectors so far + partials of the live rows
    int m = NHV + KP;
    for (int j = 0; j + 2 < KP; ++j) {
      const int need = hv_off(j + 1) + (j < J0T ? (NB - j / 4) * PLD
                                                : (NB2 - (j - J0T) / 2) * PLD2);
      m = need > m ? need : m;
    }
    if (J0T < KP) {  // the packed tail at the switch (in the 2x2 partials' place)
      const int need = hv_off(J0T) + NB2 * PLD2;
      m = need > m ? need : m;
    }
    return m;
  }
  static constexpr int REG = cap();
  static constexpr int pb_base(int J) { return REG - (NB - J) * PLD; }
  static constexpr int pb2_base(int J2) { return REG - (NB2 - J2) * PLD2; }
  union {
    ColumnChunk<KP, kTqChunk, TqStage, kTqMfmaAssembly ? MfmaLayout<KP>::PITCH : KP,
                kTqMfmaAssembly && MfmaLayout<KP>::SWZ, kTqMfmaAssembly && MfmaLayout<KP>::XSW> ch;
    double ah[KP / 2][KP + 2];            // half of A on its way from MFMA tiles to blocks
    double reg[REG];                      // hv[0, NHV) | y after the loop | pb
  } u;
  double col[KP];                         // pivot column of the current step
  double vb[KP];                          // v of the current step (zero above the pivot)
  double wb[KP];                          // w of the current step; Yb d before the loop
  // row i of T and the transformed vectors, one 32-B record per row so that a shifted solve
  // reads a row with one address; record KP only holds c(KP-1,KP) = 0
  double tq[KP + 1][4];                   // d_i, c(i-1,i), (Q^T b1)_i, (Q^T x')_i
  double tau[KP];                         // Householder scalars
};

// waves per SIMD the register allocation is held to (VGPR budget 512 / waves)
template <int KP>
struct TqOccupancy {
  static constexpr int kWaves = KP <= 40 ? 4 : KP <= 48 ? 3 : 2;
};

}  // namespace cwbl
