// cwbl_tq40_hit_merge.hip — the cache hits of several batches in one launch
// (CWBL_OPT_HIT_MERGE): solve_tq40_factor_kernel's block (tq40_factor_hit) over a list of
// segments.  A call that hits has no search for its solves to overlap, so one launch per
// cached batch only pays a ramp, a drain tail and an event boundary 29 times at C2
// (profiles/hit_merge.txt).
#include "cwbl_tq40_factor.h"

namespace cwbl {

// The hits of the segments seg[0 .. nseg) in one launch (HitSeg, cwbl_internal.h): row y of
// the grid is segment y.  What the segment's own launch of solve_tq40_factor_kernel would be
// given comes from one scalar load (blockIdx.y and the arguments are wave-uniform) and scalar
// arithmetic, its 64-bit bases included; within the segment the record and aux offsets stay
// the 32-bit ones.  The XCD order is taken per segment, as that launch would (over the whole
// grid it measured 0.3 % slower).  Working the segment out from the batch size instead of
// loading it, where the batches are equal, measured the same as the load.
// The block is the LEAN form of that text (cwbl_tq40_factor.h): the same expressions on the
// same bits with fewer VALU instructions around them (profiles/hit_lean.txt); the per-batch
// kernel and the fill keep the plain form and their register figures.  info holds what the
// fill's solves stored, so a solved point's level is read, not derived (cuts: HitLevelCuts,
// cwbl_internal.h; profiles/hit_masks.txt).
template <int KP>
__global__ void __launch_bounds__(64, 2)
solve_tq40_factor_merged_kernel(SolveConsts c, SlabDev slab, const HitSeg *__restrict__ seg,
                                const double *__restrict__ ws, const double *__restrict__ aux,
                                int2 *__restrict__ info, HitLevelCuts cuts) {
  const HitSeg sg = seg[blockIdx.y];
  const int nblk = (sg.ns + 3) >> 2;
  if ((int)blockIdx.x >= nblk) return;  // (the whole block: a row is as wide as the largest segment)
  tq40_factor_hit<KP, true>(c, slab, sg.g0, sg.ns,
                            ws + (size_t)sg.ord * FactorRecord<KP>::WORDS,
                            aux + (size_t)sg.ord * FactorAux<KP>::WORDS, info + sg.info,
                            blockIdx.x, nblk, cuts);
}

hipError_t launch_solve_tq40_factor_merged(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                           const HitSeg *seg, int nseg, int maxns,
                                           const double *ws, const double *aux, int2 *info,
                                           HitLevelCuts cuts) {
  if (nseg <= 0 || maxns <= 0) return hipSuccess;
  if (c.quad_r == nullptr || aux == nullptr || seg == nullptr || kp != kTq4KP || nseg > 65535 ||
      maxns > (1 << 19))
    return hipErrorInvalidValue;
  const dim3 grid((maxns + 3) / 4, nseg);
  hipLaunchKernelGGL((solve_tq40_factor_merged_kernel<kTq4KP>), grid, dim3(64), 0, s, c, slab,
                     seg, ws, aux, info, cuts);
  return hipGetLastError();
}

}  // namespace cwbl
