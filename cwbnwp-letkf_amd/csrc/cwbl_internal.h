// cwbl_internal.h — data layouts shared by the host orchestration (cwbl_abi.hip),
// the host k-d tree builder (kdtree_build.cpp) and the HIP kernels (cwbl_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cwbl {

// One node of a flattened kdtree2 tree (module_kdtree2.f90:512-528).  64 bytes.
struct TreeNode {
  float cut_val, cut_val_left, cut_val_right;
  int   cut_dim;          // 0..2 for internal nodes, -1 for terminal (bucket) nodes
  float lo[3];            // node%box(:)%lower (final, union of children)
  float hi[3];            // node%box(:)%upper
  int   left, right;      // child node indices (-1 = null)
  int   l, u;             // inclusive range into the permuted data
  int   pad_[2];
};
static_assert(sizeof(TreeNode) == 64, "TreeNode layout");

// Host-side result of building one tree.
struct HostTree {
  int dim = 3;
  int n = 0;
  std::vector<TreeNode> nodes;     // root = 0
  std::vector<int>      ind;       // permutation (0-based obs index of rearranged slot)
  std::vector<float>    rdata;     // rearranged normalised coords, 4 floats per slot
};

// kdtree2_create(xyz(3,n), dim) with the reference's settings (bucket 12, exact median,
// rearranged data).  xyz3 is already normalised by hclr/vclr as in build_tree.
void build_kdtree(const float *xyz3, int n, int dim, HostTree &out);

// Per-tree descriptor handed to the kernels (device-resident array of these).
struct TreeDesc {
  const TreeNode *nodes;
  const float4   *rdata;      // rearranged normalised coords (x,y,z,0)
  const int      *ind;
  // column table of this type for the current variable, one column per (tree slot,
  // obs-var): column slot*nvar + v belongs to obs ind[slot].  With the device-built index
  // (CWBL_OPT_INDEX = 1) a slot is the obs index itself: the solve's table then has rdata in
  // obs order, and the tree searches get a second table with the tree's own rdata.  Under
  // CWBL_OPT_INDEX_ORDER = 1 a slot is the position in the bins' cell-sorted order: the solve's
  // rdata is bxyz itself (no reader of the solve's table uses an entry's fourth component), and
  // the tree searches' ind is the tree's permutation composed with the positions.
  const float    *col_bg;     // [n*nvar][KP] fp32 bg = hdxb - mean, zero padded
  const float    *col_omm;    // [n*nvar] obs - mean
  const float    *col_err;    // [n*nvar] error * err_muti
  const uint8_t  *col_ok;     // [n*nvar] accepted (is_assim, qc, gross-error tests)
  float hclr_inv, vclr_inv;   // this type's own normalisation (get_lz)
  int   tree_dim;             // dimension the tree was built with
  int   query3d;              // this type queries in 3-D (own vclr > 0)
  int   nvar;
  int   max_lz;
  int   list_off;             // offset of this type inside a point's neighbour list
  int   q1_undef;
  // uniform bins over the same normalised coordinates (search_binned_kernel): cell
  // (ix, iy, iz) = floor((x - b0) * binv) per dimension, cells x-fastest; bxyz holds the
  // points cell by cell (tree-slot order within a cell) with the slot in .w (int bits),
  // bstart[c] .. bstart[c + 1] the points of cell c
  const float4 *bxyz;
  const int    *bstart;
  float bx0, by0, bz0, binv;
  int   nbx, nby, nbz;
};

// Host-side bins of one tree (build_bins, kdtree_build.cpp).
struct HostBins {
  float x0 = 0.0f, y0 = 0.0f, z0 = 0.0f, binv = 1.0f;
  int nbx = 1, nby = 1, nbz = 1;
  std::vector<float> xyzs;   // 4 floats per point: x, y, z, slot (int bits)
  std::vector<int> start;    // ncells + 1
};
// Bins of side ~r/2 (r: the search radius in normalised units) over a built tree's
// rearranged coordinates; dim 2 ignores z.  Capped at 2^22 cells.
void build_bins(const HostTree &t, int dim, float r, HostBins &out, int div = 2);
// The grid of build_bins from the coordinates' bounds (lo/hi per coordinate over its finite
// values, 0 where there is none): cell side h = r / div, grown by 1.25 until the grid has at
// most 2^22 cells; fills x0..nbz of `out`.  Shared by the host and the device bin builds.
void bin_grid(const float lo[3], const float hi[3], int dim, float r, int div, HostBins &out);

// ---- device bin build (cwbl_index.hip; CWBL_OPT_INDEX = 1 and cwbl_bin_index) ----------------
struct IndexGrid {  // HostBins' grid as the kernels take it
  float x0, y0, z0, binv;
  int nbx, nby, nbz;
};
constexpr int kIndexBoundWords = 12;
struct IndexBounds {
  float lo[3], hi[3];    // per coordinate over its finite values (build_bins), 0 if none
  float alo[3], ahi[3];  // over the points whose coordinates are all finite (bin_div_for)
  bool aseen;            // there is such a point
};
int index_bound_blocks(int n);  // blocks of launch_index_normalize: kIndexBoundWords floats each
int index_sort_blocks(int n);   // blocks of a sort pass: 256 ints of `hist` each
// xyz(3,n) -> ncoord[n] = (x hinv, y hinv, dim 3 ? z vinv : 0, 0) and the blocks' partial bounds
hipError_t launch_index_normalize(hipStream_t s, const float *xyz, int n, int dim, float hinv,
                                  float vinv, float4 *ncoord, float *part);
void index_finish_bounds(const float *part, int nblocks, IndexBounds &b);  // host
// cell ids of ncoord on grid g, then the stable sort of (cell id, obs index) by cell id:
// keys/vals are two buffers of n ints each, the result is in keys[*which], vals[*which]
hipError_t launch_index_sort(hipStream_t s, int n, int ncell, const float4 *ncoord, int dim,
                             IndexGrid g, int *keys[2], int *vals[2], int *hist, int *which);
// bstart[0..ncell] from the sorted cell ids and (bxyz non-null) the bin payload of n + kBinPad
// points: the obs index, or (by_position) the sorted position itself
hipError_t launch_index_finish(hipStream_t s, const float4 *ncoord, int n, int ncell,
                               const int *skeys, const int *svals, float4 *bxyz, int *bstart,
                               bool by_position = false);
// CWBL_OPT_INDEX_ORDER = 1: rank[order[p]] = p for the sorted obs indices order[0..n), and a
// tree's ind as sorted positions, ind2[i] = rank[ind[i]]
hipError_t launch_index_rank(hipStream_t s, const int *order, int n, int *rank);
hipError_t launch_index_compose(hipStream_t s, const int *ind, const int *rank, int n, int *ind2);

// Per-variable constants of the solve.
struct SolveConsts {
  int   k;
  int   kp;                   // padded member count of the kernel instantiation
  int   ntrees;
  int   list_cap;             // sum of max_lz over trees
  int   weight_function;
  int   use_rtpp, use_rtps;
  float inflat, rtpp_alpha, rtps_alpha;
  float nmember_inv;          // 1.0/k (module_param.f90:245)
  float r2;                   // gc1999**2
  int   max_sweeps;           // Jacobi sweep cap (CWBL_DEBUG_MAX_SWEEPS overrides; ablation only)
  const double2 *quad;        // = quad_r (non-null once the tables are built)
  const double2 *quad_r;      // [4][kQuadLevels][kQuadStride] (t2, w) of the x^-1/2 rules of
                              // 8 R - 1 nodes, R = 2, 3, 4, 8 (quad_rule)
  int   debug_stop;           // CWBL_DEBUG_TQ_STOP: 1 = after assembly, 2 = after
                              // tridiagonalisation, 3 = after quadrature, 4 = after the first
                              // kTq40J0 steps of solve_tq40_kernel (timing ablation only)
  int   debug_steps;          // CWBL_DEBUG_TQ_STEPS: > 0 runs only that many Householder steps
                              // in solve_tq_big_kernel (timing ablation only)
};
// The timing-ablation exits read debug_stop / debug_steps only in `make DEBUG_KNOBS=1`
// builds; in the release library they are the constant 0 and the branches compile away.
#ifdef CWBL_DEBUG_KNOBS
#define CWBL_DBG_STOP(c) ((c).debug_stop)
#define CWBL_DBG_STEPS(c) ((c).debug_steps)
#else
#define CWBL_DBG_STOP(c) 0
#define CWBL_DBG_STEPS(c) 0
#endif

// Inverse-square-root quadrature of the tq kernels (quad_tables.cpp): level L = 1..kQuadLevels
// covers spectrum bounds with max/min <= 10^L.  The one-wavefront kernels run kQuadNodes nodes
// per pass (64 lanes = 32 nodes x 2 sides, node 31 of the first pass the exact T^-1 solve):
// one pass (31 nodes) up to level kQuadLevels31, two (63 nodes) above; beyond 10^24 a point is
// counted non-converged.  Tables hold kQuadStride (t2, w) entries per level.
constexpr int kQuadNodes = 31;
constexpr int kQuadLevels = 24;
constexpr int kQuadLevels31 = 12;
constexpr int kQuadStride = 64;
void quad_table(int level, double2 *out64, int nodes = kQuadNodes);
// Rounds of 8 nodes (the last round's slot 7 is the exact T^-1 solve) solve_tq40_kernel runs
// at a level: the fewest whose (8 R - 1)-node rule stays within 1e-12 relative error where the
// 31-node rule does (levels 1..7), and the 31-node rule itself up to level 12, 63 nodes above
// (tests/test_quadrature.py: 15 nodes <= 2.1e-13 to level 3, 23 nodes <= 6.4e-14 to level 5).
// r6: 15 nodes at level 3 (C2: two thirds of the points, so nearly every wave of four) instead
// of 23 — one quadrature round fewer per wave; the error stays ~1e7 below the fp32 rounding of
// the analysis.
__host__ __device__ constexpr int quad_rounds(int level) {
  return level <= 3 ? 2 : level <= 5 ? 3 : level <= kQuadLevels31 ? 4 : 8;
}
// passes of the one-wavefront kernels' rule (31 nodes per pass + the exact solve)
__host__ __device__ constexpr int quad_passes(int level) { return level <= kQuadLevels31 ? 1 : 2; }
// the (8 R - 1)-node rule of a level, R = 2, 3, 4 or 8
__host__ __device__ inline const double2 *quad_rule(const double2 *quad_r, int R, int level) {
  return quad_r + ((size_t)(R == 8 ? 3 : R - 2) * kQuadLevels + (level - 1)) * kQuadStride;
}

// Point enumeration of a slab: g = i + ix_lim*(j + iy_lim*kz).
struct SlabDev {
  int nx, ny, nz, alt_nx, alt_ny, ix_lim, iy_lim;
  long long L;                // nx*ny*nz (member stride of var)
  const float *x, *y, *alt;
  float *var;
};

// Device-side counters (atomics) reported through cwbl_stats.
struct DevStats {
  unsigned long long solved, nobs_sum, lz_truncated, nonconverged, q1_undefined, sweeps_sum;
  unsigned int max_p, max_sweeps;
};

// Kernel launchers (cwbl_kernels.hip).
hipError_t launch_obs_prep(hipStream_t s, int k, int kp, int family, int type_id, int nvar,
                           int nobs, const float *obs, const float *error, const float *hdxb,
                           const int *qc, const float err_muti[5], const float err_rej[5],
                           const int is_assim[5], float norain, const int *slot_obs,
                           float *col_bg, float *col_omm, float *col_err, uint8_t *col_ok);

// Cyclic (block 1) column decomposition of letkf_local_info (module_mpi_util.f90:71-188) on a
// px x py rank grid: rank r = id_x + id_y*px owns x = id_x + i*px, y = id_y + j*py.
constexpr int kMaxRankDim = 64;
struct Decomp {
  int nx, ny, nz, px, py;
  int cols_before[kMaxRankDim];  // columns owned by rank coordinates a < id_x
  int rows_before[kMaxRankDim];  // rows owned by rank coordinates b < id_y
};
void make_decomp(Decomp &d, int nx, int ny, int nz, int px, int py);
hipError_t launch_pack_columns(hipStream_t s, const float *global, const Decomp &d,
                               float *send);
hipError_t launch_unpack_columns(hipStream_t s, const float *recv, const Decomp &d,
                                 float *global);
// nm member fields at once (member i at src + i sstride -> dst + i dstride, in elements)
hipError_t launch_transpose_columns(hipStream_t s, bool unpack, const float *src,
                                    long long sstride, int nm, const Decomp &d, float *dst,
                                    long long dstride);
hipError_t launch_vcoord_mean(hipStream_t s, const float *ph, long long n2d, int nz_ph, int k,
                              int stagger, float alpha, float *alt);
hipError_t launch_member_sum(hipStream_t s, const float *fields, long long n, int nm,
                             float *out);
hipError_t launch_scale(hipStream_t s, float *x, long long n, float alpha);

// letkf_tune_q over the analysed region of s.var (module_letkf_core.f90:702-733)
hipError_t launch_tune_q(hipStream_t st, SlabDev s, int k);
// ... over nrun runs of n points of that region, run r from point g0 + r * stride (a batch of
// a piped host slab: one run; a column batch of a column-shared call: one run per level,
// stride = ix_lim * iy_lim).  hipErrorInvalidValue when a run leaves the region.
hipError_t launch_tune_q_range(hipStream_t st, SlabDev s, int k, long long g0, long long n,
                               int nrun = 1, long long stride = 0);

// depth: the deepest tree's level count (tree_depth), which sizes the traversal stacks.
// obs_slots (CWBL_OPT_INDEX = 1): the columns are numbered by obs index, so the analysis lists
// get ind[slot] instead of the tree slot, and a type without a tree (nodes == nullptr: it
// cannot truncate) keeps the list the binned search wrote.
hipError_t launch_search(hipStream_t s, const TreeDesc *trees, int ntrees, int depth,
                         int list_cap, float r2, SlabDev slab, long long g0, int npts,
                         int *nbr_cnt, int *nbr_idx, float *nbr_r2, DevStats *stats,
                         bool obs_slots = false);

// nbr_idx holds tree slots (search with nbr_r2 = nullptr); the solve recomputes r2
hipError_t launch_solve_neighbors(hipStream_t s, int kp, const TreeDesc *trees,
                                  SolveConsts c, SlabDev slab, long long g0, int npts,
                                  const int *nbr_cnt, const int *nbr_idx, int2 *info);

hipError_t launch_solve_assembled(hipStream_t s, int kp, SolveConsts c, int npts,
                                  const long long *col_off, const float *yo, const float *yb,
                                  const float *xb, float *xa, double *evals, int2 *info);

// Tridiagonalisation + quadrature solve (cwbl_tq.hip); same data contract as the two
// launchers above.  `tri` (assembled mode only): T of every point for launch_tridiag_eigvals.
hipError_t launch_solve_tq(hipStream_t s, int kp, bool assembled, const TreeDesc *trees,
                           SolveConsts c, SlabDev slab, long long g0, int npts,
                           const int *nbr_cnt, const int *nbr_idx,
                           const long long *col_off, const float *yo, const float *yb,
                           const float *xb, float *xa, int2 *info, double *tri = nullptr);

constexpr int kTq4KP = 40;  // KP of the split record path (k = 25..40)

// The default KP = 40 split: assemble_record_kernel (cwbl_tq.hip) only stages and assembles,
// one point per wavefront, and writes A = inflat I + Yb Yb^T (packed lower, the padding's
// diagonal 1) and b1 = Yb d; solve_tq40_kernel (cwbl_tq40.hip) runs the whole
// tridiagonalisation with four points per wavefront (the first kTq40J0 steps on full rows
// J0..KP-1 plus the prefix rows' top-left block, then 16-lane rows of the trailing 32 x 32
// matrix), solves and writes var in place.
constexpr int kTq40J0 = 8;
constexpr int kRecordWaves = 4;  // waves per SIMD of the record kernel (assemble_record_kernel)
template <int KP>
struct AsmRecord {
  static constexpr int TA = 0;                   // A(r, c), c <= r, at r (r + 1) / 2 + c
  static constexpr int U1 = KP * (KP + 1) / 2;   // b1 = Yb d (KP)
  static constexpr int WORDS = (U1 + KP + 1) / 2 * 2;
};
// What the record cache keeps of a point under CWBL_OPT_FACTOR_REUSE, in the record's own
// words: the factor A = Q T Q^T as LAPACK's dsytrd stores it, with step j's scal (the factor
// dlarfg scales x by) where dsytrd would put e_j, and Q^T b1.  Column j = 0 .. KP-3 is stored by
// row, rows j + 1 .. KP-1 (scal_j, then the unscaled, masked pivot column x), so that the 16
// lanes of a DPP row read 16 consecutive words; scal_j lies where solve_tq40_multi_kernel's
// layout keeps it (word 0 of sm.pv's column in phase 1, row j + 1 of the column's registers in
// phase 2).  T's off-diagonal and the steps' tau are the point's FactorAux.
template <int KP>
struct FactorRecord {
  static constexpr int D = 0;         // diagonal of T (KP)
  static constexpr int U1 = KP;       // Q^T b1 (KP)
  static constexpr int COL = 2 * KP;  // the columns
  // row j + 1 of column j; row i >= j + 1 at col(j) + i - (j + 1)
  static constexpr int col(int j) { return COL + j * (KP - 1) - j * (j - 1) / 2; }
  static constexpr int EL = col(KP - 2);  // unused (FactorAux::B holds c(KP-2, KP-1)): keeps WORDS
  static constexpr int WORDS = EL + 1;
};
static_assert(FactorRecord<kTq4KP>::WORDS == AsmRecord<kTq4KP>::WORDS,
              "a factor takes its record's slot");
// The steps' scalars of a cached factor, an entry per record in a buffer of its own (same
// ordinal as the record): the bits the fill's dlarfg produced, so that a hit runs none.
//   B + i: T's off-diagonal as sm.tq[q][i][1] holds it: 0 at i = 0, beta_{i-1} for
//          i = 1 .. KP-2, the trailing c(KP-2, KP-1) at KP-1;
//   T + j: tau_j as sm.tau[q][j] holds it, 0 for j = KP-2 and KP-1.
// Lane l of a point's row reads words l, l + 16, ... of each half: a wave's four entries are
// 4 WORDS contiguous words.
template <int KP>
struct FactorAux {
  static constexpr int B = 0;
  static constexpr int T = KP;
  static constexpr int WORDS = 2 * KP;
};
hipError_t launch_assemble_record(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                                  SlabDev slab, long long g0, int npts, const int *nbr_cnt,
                                  const int *nbr_idx, int2 *info, double *ws);
hipError_t launch_solve_tq40(hipStream_t s, int kp, SolveConsts c, SlabDev slab, long long g0,
                             int npts, double *ws, int2 *info);
// The record cache's pair (cwbl_tq40_fill.hip): fill_tq40_factor_kernel is solve_tq40_kernel's
// analysis from the records `ws`, which it leaves as FactorRecords; solve_tq40_factor_kernel is
// the same analysis from those.  Same launch contract as launch_solve_tq40 (the spare record
// included); aux: the FactorAux entries of the npts + 1 records `ws` (the fill writes those of
// the npts points, the hit's lanes past the launch read the spare one).
hipError_t launch_fill_tq40_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   long long g0, int npts, double *ws, double *aux, int2 *info);
hipError_t launch_solve_tq40_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                    long long g0, int npts, const double *ws, const double *aux,
                                    int2 *info);

// One launch for the hits of several cached batches (CWBL_OPT_HIT_MERGE): what
// launch_solve_tq40_factor does once per segment, a segment being what one of its launches
// covers (a cached batch, or a sub-batch of one).  Segment y is row y of a two-dimensional
// grid, so that no wave holds points of two segments and the waves of a segment group its
// points as its own launch would; the row is as wide as the largest segment, and the blocks
// past a shorter one's last wave leave at once.
struct HitSeg {
  long long g0;   // first point
  long long ord;  // ordinal of its first record and FactorAux entry in `ws` and `aux`; its
                  // spare ones are at ord + ns
  int ns;         // points (<= 2^19)
  int info;       // its info from info[info]
};
// The merged hit takes a solved point's level from the info the fill kept, and needs the trace
// only for the lanes that have none (p = 0, past the segment), whose level reaches nothing but
// the wave's rounds: t[i] is the smallest trace(T) from which solve_tq40_kernel's level loop
// ends above kRoundCuts[i], the levels after which quad_rounds steps (NaN: no trace does).
constexpr int kRoundCuts[3] = {3, 5, kQuadLevels31};
static_assert(quad_rounds(1) == quad_rounds(kRoundCuts[0]) &&
              quad_rounds(kRoundCuts[0] + 1) == quad_rounds(kRoundCuts[1]) &&
              quad_rounds(kRoundCuts[1] + 1) == quad_rounds(kRoundCuts[2]) &&
              quad_rounds(kRoundCuts[2] + 1) == quad_rounds(kQuadLevels),
              "quad_rounds steps after kRoundCuts only");
struct HitLevelCuts {
  double t[3];
};
// seg: the nseg <= 65535 segments, on the device; maxns: the largest one's points; info: as
// restore_info left it (p, and the fill's +-level where p > 0).
hipError_t launch_solve_tq40_factor_merged(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                           const HitSeg *seg, int nseg, int maxns,
                                           const double *ws, const double *aux, int2 *info,
                                           HitLevelCuts cuts);

// cwbl_analyze_vars: the variables of a group share the record (A, b1) and so the factor
// A = Q T Q^T; solve_tq40_multi_kernel (cwbl_tq40_multi.hip) tridiagonalises once per point
// and replays the reflectors on every variable's x'.  The per-variable table goes to the
// kernel by value; slab.var is unused there.
constexpr int kMaxGroupVars = 8;  // = CWBL_MAX_GROUP_VARS
struct Tq40Vars {
  float *var[kMaxGroupVars];
  float rtpp_alpha[kMaxGroupVars], rtps_alpha[kMaxGroupVars];
  int use_rtpp[kMaxGroupVars], use_rtps[kMaxGroupVars];
  int nvar;
};
hipError_t launch_solve_tq40_multi(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   const Tq40Vars &vars, long long g0, int npts, double *ws,
                                   int2 *info);

// CWBL_OPT_COLUMN_SHARE = 1 on the record path: the records are those of the slab's columns
// (the points kz = 0: a 2-D localisation gives every level of a column the same A and b1), and
// solve_tq40_column_kernel (cwbl_tq40_column.hip) tridiagonalises once per column and replays
// the reflectors on the x' of every level.  slab is the whole slab (var, nx, ny, L), g0 and
// npts count columns; the launch is (ceil(npts / 4), ceil(nz / lw)) with lw levels per wave.
hipError_t launch_solve_tq40_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                    long long g0, int npts, int nz, int lw, double *ws,
                                    int2 *info);

// The group call of the one-wavefront path (k <= 16, 41..64, and 17..40 without the record
// split): solve_tq_multi_kernel<KP, NV> (cwbl_tq_multi.hip) is solve_tq_kernel<KP, false> with
// the x' of up to NV variables carried through one tridiagonalisation.  NV is the class of
// the group's size (unused slots carry zeros); the same data contract as launch_solve_tq's
// slab mode, with the variables' table in place of slab.var.  nvar >= 2.
constexpr int group_var_class(int nvar) { return nvar <= 2 ? 2 : nvar <= 4 ? 4 : 8; }
hipError_t launch_solve_tq_multi(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                                 SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                 const int *nbr_cnt, const int *nbr_idx, int2 *info);

// Split form of the KP = 128 slab path (configs[3]: k = 97..128).  solve_tq_big_kernel<128,
// false, kBigJ0> assembles A and runs the first kBigJ0 Householder steps (4x4 register
// blocks over 256 threads, one point per workgroup), then hands the trailing
// (KP-J0)^2 matrix, its J0 reflectors, T so far and Q^T b1, Q^T x' over through the
// workspace (BigHandoff, info[gi] = (p, 0)); solve_tqb_tail_kernel (cwbl_tq_tail.hip)
// finishes with one point per wavefront, lane l holding the full trailing row J0 + l.
// (KP = 96, k = 65..96: the same with the hand-off after 32 steps)
constexpr int kBigSplitKP = 128;
constexpr int kBigJ0 = 64;
constexpr int big_split_j0(int kp) { return kp - 64; }
// fp64 words of one point's hand-off record
template <int KP, int J0>
struct BigHandoff {
  static constexpr int KT = KP - J0;        // trailing rows
  static constexpr int TA = 0;              // trailing A, full: (r, c) at TA + c*KT + r
  static constexpr int HV = TA + KT * KT;   // reflector j < J0 at HV + j*KP + row (rows > j)
  static constexpr int D = HV + J0 * KP;    // d_0 .. d_{J0-1}
  static constexpr int E = D + J0;          // c(j, j+1), j = 0..J0-1
  static constexpr int TAU = E + J0;        // tau_0 .. tau_{J0-1}
  static constexpr int U1 = TAU + J0;       // Q_J0^T b1 (KP)
  static constexpr int U2 = U1 + KP;        // Q_J0^T x' (KP)
  static constexpr int BT = U2 + KP;        // tail scratch: its reflector rows (KT x KT)
  static constexpr int WORDS = BT + KT * KT;
};
hipError_t launch_big_handoff(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                              SlabDev slab, long long g0, int npts, const int *nbr_cnt,
                              const int *nbr_idx, int2 *info, double *ws);
// KP = 128: the half-row hand-off kernel (cwbl_tq_rows.hip), launched by launch_big_handoff
hipError_t launch_rows_handoff(hipStream_t s, const TreeDesc *trees, SolveConsts c, SlabDev slab,
                               long long g0, int npts, const int *nbr_cnt, const int *nbr_idx,
                               int2 *info, double *ws);
hipError_t launch_solve_tqb_tail(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                 long long g0, int npts, double *ws, int2 *info);

// The group call of the hand-off path (k = 65..128, cwbl_analyze_vars with two or more
// variables): solve_tq_rows_multi_kernel<128, 64, NV> (cwbl_tq_rows_multi.hip) and
// solve_tq_big_multi_kernel<96, 32, NV> (cwbl_tq_big_multi.hip) are the hand-off kernels with
// the x' of up to NV variables carried through the steps, solve_tqb_tail_multi_kernel<KP, J0,
// NV> (cwbl_tq_tail_multi.hip) the tail kernel likewise, which then solves variable by
// variable.  The record is BigHandoff's with the further variables' Q^T x' appended, so that
// every word the single kernels address keeps its place.
template <int KP, int J0, int NV>
struct BigHandoffMulti : BigHandoff<KP, J0> {
  using Base = BigHandoff<KP, J0>;
  static constexpr int U2X = Base::WORDS;  // Q_J0^T x' of variables 1 .. NV-1 (KP each)
  static constexpr int WORDS = U2X + (NV - 1) * KP;
  // Q_J0^T x' of variable i
  __host__ __device__ static constexpr int u2(int i) { return i == 0 ? Base::U2 : U2X + (i - 1) * KP; }
};
// fp64 words of a point's record on the hand-off path: a single call's (nv <= 1) or a group's
// of class nv (group_var_class)
constexpr size_t big_handoff_words(int kp, int nv) {
  return (size_t)(kp == 96 ? BigHandoff<96, 32>::WORDS : BigHandoff<kBigSplitKP, kBigJ0>::WORDS) +
         (size_t)(nv > 1 ? nv - 1 : 0) * kp;
}
hipError_t launch_big_handoff_multi(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                                    SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                    const int *nbr_cnt, const int *nbr_idx, int2 *info,
                                    double *ws);
hipError_t launch_rows_handoff_multi(hipStream_t s, const TreeDesc *trees, SolveConsts c,
                                     SlabDev slab, const Tq40Vars &vars, long long g0, int npts,
                                     const int *nbr_cnt, const int *nbr_idx, int2 *info,
                                     double *ws);
hipError_t launch_solve_tqb_tail_multi(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                       const Tq40Vars &vars, long long g0, int npts, double *ws,
                                       int2 *info);

// The factor cache of the one-wavefront path at KP = 48, 56, 64 (CWBL_OPT_WAVE_REUSE,
// cwbl_tq_wave.hip).  What it keeps of a point, in fp64 words: T's diagonal and off-diagonal
// as sm.tq[i][0] and sm.tq[i][1] hold them after solve_tq_kernel's loop, Q^T b1, and per step j
// tau_j, the factor scal_j that dlarfg scales x by (both the bits the fill's dlarfg returned) and
// the unscaled, masked pivot column x: rows j + 1 .. KP-1 (row j + 1 is 0) as consecutive words,
// one per lane.  A hit forms v = x scal where the single kernel forms it.
template <int KP>
struct WaveFactor {
  static constexpr int D = 0;           // d_i (KP)
  static constexpr int C = KP;          // c(i-1, i): 0 at i = 0 (KP)
  static constexpr int U1 = 2 * KP;     // Q^T b1 (KP)
  static constexpr int TAU = 3 * KP;    // tau_j, 0 for a step that ran no reflector (KP)
  static constexpr int SCAL = 4 * KP;   // scal_j (KP; unwritten where step j left early)
  static constexpr int COL = 5 * KP;    // the columns
  // row j + 1 of column j; row i >= j + 1 at col(j) + i - (j + 1)
  __host__ __device__ static constexpr int col(int j) {
    return COL + j * (KP - 1) - j * (j - 1) / 2;
  }
  static constexpr int WORDS = KP * (KP - 1) / 2 + 5 * KP;
};
static_assert(WaveFactor<64>::col(63) == WaveFactor<64>::WORDS, "the columns fill the factor");
constexpr size_t wave_factor_words(int kp) {
  return kp == 48 ? WaveFactor<48>::WORDS : kp == 56 ? WaveFactor<56>::WORDS
                                                      : WaveFactor<64>::WORDS;
}
// fill: launch_solve_tq's slab mode, which also leaves the npts factors at `fac`; the hit: the
// same analysis from them and from info[i].x = p of the fill (no lists, no trees).
hipError_t launch_fill_tq_wave(hipStream_t s, int kp, const TreeDesc *trees, SolveConsts c,
                               SlabDev slab, long long g0, int npts, const int *nbr_cnt,
                               const int *nbr_idx, int2 *info, double *fac);
hipError_t launch_solve_tq_wave_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                       long long g0, int npts, const double *fac, int2 *info);

// The factor cache of the hand-off path at KP = 96 (CWBL_OPT_BIG_REUSE, cwbl_tq_big_factor.hip).
// What it keeps of a point, in fp64 words, every one the bits the fill's kernel pair produced:
// T's diagonal and off-diagonal, Q^T b1, tau_j and (steps j >= J0) scal_j as the tail's sm.tq,
// sm.tau and sm.scl hold them after its loop; the hand-off kernel's reflectors j < J0 as it
// forms them (v_j = x scal with 1 at row j + 1: BigHandoff::HV), rows j + 1 .. KP-1; the tail's
// columns j >= J0 as the raw pivot row x (BigHandoff::BT), rows j + 2 .. KP-1.  The two halves
// differ because the kernels do: the hand-off kernel sums v . x', the tail scal (x . x') + x'_{j+1}.
// A column's rows are consecutive words, one per lane.
template <int KP, int J0>
struct BigFactor {
  static constexpr int KT = KP - J0;
  static constexpr int D = 0;           // d_i (KP)
  static constexpr int C = KP;          // c(i-1, i) as sm.tq[i][1]: 0 at i = 0 (KP)
  static constexpr int U1 = 2 * KP;     // Q^T b1 (KP)
  static constexpr int TAU = 3 * KP;    // tau_j (KP)
  static constexpr int SCAL = 4 * KP;   // scal_j, j = J0 .. k-3 (KP; the others unwritten)
  static constexpr int HV = 5 * KP;     // the hand-off kernel's reflectors
  // row j + 1 of reflector j < J0; row i >= j + 1 at hv(j) + i - (j + 1)
  __host__ __device__ static constexpr int hv(int j) { return HV + j * (KP - 1) - j * (j - 1) / 2; }
  static constexpr int BT = hv(J0);     // the tail's columns
  // row J0 + jl + 2 of the tail's step jl (j = J0 + jl); row J0 + l, l >= jl + 2, at
  // bt(jl) + l - (jl + 2)
  __host__ __device__ static constexpr int bt(int jl) {
    return BT + jl * (KT - 2) - jl * (jl - 1) / 2;
  }
  static constexpr int WORDS = bt(KT - 2);
};
static_assert(BigFactor<96, 32>::WORDS <= 96 * 95 / 2 + 5 * 96, "the factor's bound");
// KP = 128 (CWBL_OPT_ROWS_REUSE, cwbl_tq_rows_factor.hip): the same struct over the half-row
// hand-off kernel's 64 reflectors, 640 + 6112 + 1953 = 8705 words
static_assert(BigFactor<128, 64>::WORDS <= 128 * 127 / 2 + 5 * 128, "the factor's bound");
constexpr size_t big_factor_words(int kp) {
  return kp == 96 ? BigFactor<96, 32>::WORDS : kp == 128 ? BigFactor<128, 64>::WORDS : 0;
}
// fill: launch_solve_tqb_tail on the hand-off kernel's records `ws`, which also leaves the npts
// factors at `fac`; the hit: the same analysis from them and from info[i].x = p of the fill (no
// lists, no trees, no hand-off kernel, no records).  KP = 96 (cwbl_tq_big_factor.hip) and
// KP = 128 (launch_*_rows, cwbl_tq_rows_factor.hip, which the two launchers pass on to).
hipError_t launch_fill_tqb_tail(hipStream_t s, int kp, SolveConsts c, SlabDev slab, long long g0,
                                int npts, double *ws, int2 *info, double *fac);
hipError_t launch_solve_tqb_factor(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                   long long g0, int npts, const double *fac, int2 *info);
hipError_t launch_fill_tqb_tail_rows(hipStream_t s, SolveConsts c, SlabDev slab, long long g0,
                                     int npts, double *ws, int2 *info, double *fac);
hipError_t launch_solve_tqb_factor_rows(hipStream_t s, SolveConsts c, SlabDev slab, long long g0,
                                        int npts, const double *fac, int2 *info);

// A column-shared call's levels from kept factors (CWBL_OPT_COLUMN_FACTOR): the fill above has
// analysed level 0 of the ncol columns from g0 on the column view and left their factors at
// `fac` and their accepted counts in info[i].x; these solve the levels 1 .. nz-1 of every column
// from its factor, one column per wavefront and lw levels per wavefront (grid (ncol,
// ceil((nz - 1) / lw)); the bits do not depend on lw).  slab is the whole slab (nz levels);
// info is read only.  cwbl_tq_wave_column.hip (KP = 48, 56, 64: solve_tq_wave_factor_kernel's
// replay and tq_wave_finish per level), cwbl_tq_big_column.hip (KP = 96: tqb_factor_hit per
// level) and cwbl_tq_rows_column.hip (KP = 128, CWBL_OPT_COLUMN_ROWS: tqb_rows_hit per level;
// launch_*_rows, which the KP launcher passes on to).
hipError_t launch_solve_tq_wave_factor_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                              long long g0, int ncol, int nz, int lw,
                                              const double *fac, const int2 *info);
hipError_t launch_solve_tqb_factor_column(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                          long long g0, int ncol, int nz, int lw,
                                          const double *fac, const int2 *info);
hipError_t launch_solve_tqb_factor_column_rows(hipStream_t s, SolveConsts c, SlabDev slab,
                                               long long g0, int ncol, int nz, int lw,
                                               const double *fac, const int2 *info);

// A column-shared call that hits the column cache (CWBL_OPT_COLUMN_REUSE): the two kernels above
// started at level 0, since no fill of this call analysed it.  `fac` and info[i].x are what an
// earlier call's fill left for the ncol columns from g0; these solve the levels 0 .. nz-1 of
// every column (grid (ncol, ceil(nz / lw))).  cwbl_tq_wave_column_all.hip (KP = 48, 56, 64),
// cwbl_tq_big_column_all.hip (KP = 96) and cwbl_tq_rows_column.hip (KP = 128).
hipError_t launch_solve_tq_wave_factor_column_all(hipStream_t s, int kp, SolveConsts c,
                                                  SlabDev slab, long long g0, int ncol, int nz,
                                                  int lw, const double *fac, const int2 *info);
hipError_t launch_solve_tqb_factor_column_all(hipStream_t s, int kp, SolveConsts c, SlabDev slab,
                                              long long g0, int ncol, int nz, int lw,
                                              const double *fac, const int2 *info);
hipError_t launch_solve_tqb_factor_column_all_rows(hipStream_t s, SolveConsts c, SlabDev slab,
                                                   long long g0, int ncol, int nz, int lw,
                                                   const double *fac, const int2 *info);

// KP = 96, 128: one 256-thread workgroup per point (cwbl_tq_big.hip)
hipError_t launch_solve_tq_big(hipStream_t s, int kp, bool assembled, const TreeDesc *trees,
                               SolveConsts c, SlabDev slab, long long g0, int npts,
                               const int *nbr_cnt, const int *nbr_idx,
                               const long long *col_off, const float *yo, const float *yb,
                               const float *xb, float *xa, int2 *info, double *tri = nullptr);

// Eigenvalues of the tridiagonal T = Q^T A Q the tq kernels form (assembled mode, `tri`:
// per point d_0..d_{KP-1} then c(i, i+1), 2 KP words): ascending, by Sturm-count bisection
// in fp64 (cwbl_eig.hip), i.e. the eigenvalues of A that dsyevd returns (module_eigen.f90:49)
hipError_t launch_tridiag_eigvals(hipStream_t s, int kp, int k, int npts, const double *tri,
                                  double *evals);

// The analysis search from uniform bins: the same fixed-radius sets as launch_search (the
// same fp32 distances and <= r2 test) in bin order, which differs from kdtree2's visiting
// order; a point whose list would pass max_lz on any tree is appended to flag_idx
// (flag_cnt, zeroed by the caller) for launch_search_flagged, which reruns the tree search
// there so Q4 truncation keeps the reference's order.  rbox: the bounding-box half-width,
// sqrt(r2) with a margin.
hipError_t launch_search_binned(hipStream_t s, const TreeDesc *trees, int ntrees, int list_cap,
                                float r2, float rbox, SlabDev slab, long long g0, int npts,
                                int *nbr_cnt, int *nbr_idx, int *flag_cnt, int *flag_idx);
hipError_t launch_search_flagged(hipStream_t s, const TreeDesc *trees, int ntrees, int depth,
                                 int list_cap, float r2, SlabDev slab, long long g0, int npts,
                                 const int *flag_cnt, const int *flag_idx, int *nbr_cnt,
                                 int *nbr_idx, DevStats *stats, bool obs_slots = false);

hipError_t launch_search_single(hipStream_t s, const TreeDesc *tree, int depth, float r2,
                                int nq, const float *q_xyz, int max_lz, int *nfound, int *idx,
                                float *r2out);

hipError_t launch_reduce_info(hipStream_t s, const int2 *info, int n, DevStats *stats);

// Record reuse: n coordinates `cur` against their snapshot `snap`, bit for bit (*flag, zeroed
// by the caller, becomes 1 on any mismatch); store: snap = cur instead (flag unused).
hipError_t launch_coord_snapshot(hipStream_t s, bool store, const float *cur, float *snap,
                                 long long n, int *flag);

constexpr int kSearchStackDepth = 40;  // max k-d tree depth the search kernel supports

// Neighbour lists of the analysis path are interleaved by groups of kListLanes points and
// kListGroup slots: slot s of point g lives at list_index(g, cap, off) + list_slot(s).  A
// search wave then stores 16 B per lane side by side (whole cache lines) instead of 64
// scattered 4-B streams, and a solve reading 32 consecutive slots of one point touches 8
// lines instead of 32.  cap and off are multiples of kListGroup (list_span); buffers hold
// round_up(npts, kListLanes) * cap entries.
constexpr int kListLanes = 64;
constexpr int kListGroup = 4;
// points of padding after a tree's bins: search_binned_kernel reads ahead past a run's end
constexpr int kBinPad = 8;
__host__ __device__ inline int list_span(int max_lz) {
  return (max_lz + kListGroup - 1) / kListGroup * kListGroup;
}
__host__ __device__ inline long long list_index(long long g, int cap, int off) {
  return (g / kListLanes) * (long long)cap * kListLanes + (long long)off * kListLanes +
         (g % kListLanes) * kListGroup;
}
__host__ __device__ inline unsigned list_slot(int s) {  // s >= 0
  return (unsigned)s / kListGroup * (kListGroup * kListLanes) + (unsigned)s % kListGroup;
}

int supported_kp(int k);      // smallest compiled KP >= k, or -1
// sets the message cwbl_last_error() returns and returns `code` (cwbl_abi.hip)
int set_last_error(int code, const char *msg);
constexpr int kMaxWaveKP = 64;  // largest KP of the one-wavefront kernels

}  // namespace cwbl
