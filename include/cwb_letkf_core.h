/*
 * cwb_letkf_core.h — C ABI of the MI355X LETKF analysis core.
 *
 * This is the drop-in boundary for the per-variable hot loop of the reference
 * LETKF (lopunch/CWBNWP-LETKF).  A Fortran host binds it with iso_c_binding
 * (see cwbnwp-letkf_amd/fortran/letkf_core_gpu.f90 and INTEGRATION.md); Python
 * binds it with ctypes (cwbnwp-letkf_amd/cwbl/abi.py).
 *
 * Entry point                reference interface it replaces
 * -------------------------  ------------------------------------------------------------
 * cwbl_init                  set_optimal_workspace_for_eigen + set_ensemble_constants
 *                            (module_eigen.f90:16-35, module_param.f90:241-247,
 *                            called at cwb_letkf.f90:37-38)
 * cwbl_set_obs               the obs state after gts%distribute / rad%distribute
 *                            (module_gts_omboma.f90:508-611, module_radar.f90:120-186),
 *                            i.e. wrfda_gts%platform(:) and cwb_radar%radarobs(:)
 * cwbl_analyze_var           one pass of letkf_driver's update loop for one variable:
 *                            build_tree x2 (module_letkf_core.f90:63-64) + the grid-point
 *                            loop (module_letkf_core.f90:209-240) + destroy_tree (:295)
 * cwbl_solve_batch           letkf_solve (module_letkf_core.f90:598-700) for many points
 *                            with pre-assembled yo/yb (KAT / diagnostics entry)
 * cwbl_search                build_tree + get_lz for one obs type
 *                            (module_localization.f90:35-167, 188-331) (KAT entry)
 * cwbl_finalize              destroy_eigen_array (module_eigen.f90:110-113)
 * cwbl_last_error            replaces `stop "<msg>"`: the library never exits
 *
 * Conventions
 *  - float <-> real(c_float), double <-> real(c_double), int <-> integer(c_int),
 *    long long <-> integer(c_long_long).  Fortran logicals cross as int 0/1.
 *  - Arrays are passed in the reference's Fortran (column-major) layout, first index
 *    fastest; the comment next to each pointer gives the Fortran shape.
 *  - Observation / result indices are 0-based on this side of the ABI.
 *  - All calls are synchronous, from one host thread per process; `memory` says whether
 *    the array pointers of a struct are host pointers (copied in/out inside the call) or
 *    HIP device pointers already resident on the library's device.
 *  - Device inputs only need to be *queued* on the caller's stream (cwbl_set_stream; the
 *    legacy null stream by default): every call that takes device pointers first makes the
 *    library's streams wait for an event recorded there, so work queued on OTHER streams
 *    (torch's non-default streams, an RCCL collective's stream) must be complete or ordered
 *    before that stream by the caller.  All library work on those buffers has completed when
 *    the call returns.
 *  - Return value 0 = success; nonzero = error code, message in cwbl_last_error().
 *  - There is no CPU fallback: without a usable gfx950 device every compute entry point
 *    returns CWBL_ERR_NO_DEVICE.
 */
#ifndef CWB_LETKF_CORE_H
#define CWB_LETKF_CORE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWBL_ABI_VERSION 2

#define CWBL_MAX_NVAR        5   /* obs variables per GTS report (u,v,t,p,q) */
#define CWBL_NUM_GTS_TYPES  29   /* module_param.f90:172 num_gts_indexes     */
#define CWBL_NUM_RADAR_TYPES 4   /* module_param.f90:212 num_radar_indexes   */
#define CWBL_MAX_MEMBERS    128  /* largest k the solve kernels support      */

/* GTS type ids (module_param.f90:143-171); only these five are assimilated
 * (module_localization.f90:59-72). */
enum {
  CWBL_GTS_SOUND = 1, CWBL_GTS_SYNOP = 2, CWBL_GTS_GPSPW = 8,
  CWBL_GTS_METAR = 10, CWBL_GTS_SHIPS = 11
};
/* radar type ids (module_param.f90:208-211) */
enum { CWBL_RADAR_DBZ = 1, CWBL_RADAR_VR = 2, CWBL_RADAR_ZDR = 3, CWBL_RADAR_KDP = 4 };

enum { CWBL_MEM_HOST = 0, CWBL_MEM_DEVICE = 1 };

enum {
  CWBL_OK = 0,
  CWBL_ERR_ARG = 1,          /* invalid argument / shape                        */
  CWBL_ERR_STATE = 2,        /* call order (e.g. analyze before init/set_obs)    */
  CWBL_ERR_NO_DEVICE = 3,    /* no HIP device / wrong architecture              */
  CWBL_ERR_HIP = 4,          /* HIP runtime error                               */
  CWBL_ERR_UNSUPPORTED = 5,  /* configuration outside this build (e.g. k > 128)  */
  CWBL_ERR_OOM = 6
};

/* Q1: build_tree picks the tree dimension from the last type appended
 * (module_localization.f90:151).  CWBL_Q1_REPLICATE follows it wherever the result is
 * defined (a 3-D type in a 2-D tree family is searched in 2-D); a 2-D type in a 3-D
 * family reads an undefined qv(3) in the reference, and is searched in 2-D with its own
 * tree (counted in cwbl_stats.q1_undefined).  CWBL_Q1_PER_TYPE uses every type's own
 * vclr for its tree. */
enum { CWBL_Q1_REPLICATE = 0, CWBL_Q1_PER_TYPE = 1 };

typedef struct cwbl_init_params {
  int    nmember;          /* k = config%nmember (module_config.f90:306), 2..128 */
  int    device;           /* HIP device ordinal, -1 = current device */
  int    weight_function;  /* 0 Gaussian, 1 Gaspari-Cohn (module_config.f90:307) */
  float  norain_value;     /* control_nml norain_value (module_config.f90:295) */
  int    q1_mode;          /* CWBL_Q1_* */
  int    reserved;
  size_t workspace_bytes;  /* device workspace budget for neighbour lists (0 = 2 GiB); the
                            * solve's per-batch records come on top: 6.9 KB per point of a
                            * search batch at k = 17..40 (two buffers); at k = 65..128 the
                            * hand-off records (135 KB per point) are bounded by this value
                            * when it is given, else by min(13 GB, 40% of the device memory
                            * free at cwbl_init), with sub-batches shrunk to fit.  The
                            * records kept for reuse at k = 17..40 (CWBL_OPT_RECORD_REUSE:
                            * 6.9 KB per point of the cached batches, 31 GB for a
                            * 300 x 300 x 50 slab) have their own budget and are outside
                            * this value too */
} cwbl_init_params;

/* One GTS platform: type(gts_structure), module_gts_omboma.f90:13-22. */
typedef struct cwbl_gts_obs {
  int          type_id;   /* CWBL_GTS_* */
  int          nvar;      /* 5 synop/metar/ships, 4 sound, 1 gpspw */
  int          nobs;
  int          reserved;
  const float *xyz;       /* xyz(3,nobs), projected metres (module_param.f90:7) */
  const float *obs;       /* obs(nvar,nobs) */
  const float *error;     /* error(nvar,nobs) */
  const float *hdxb;      /* hdxb(nvar,nobs,0:k-1) = H(x_b) per member (:171) */
  const int   *qc;        /* qc(nvar,nobs,0:k-1) */
} cwbl_gts_obs;

/* One radar variable: type(radar_structure), module_radar.f90:13-16. */
typedef struct cwbl_radar_obs {
  int          type_id;   /* CWBL_RADAR_* */
  int          nobs;
  const float *xyz;       /* xyz(3,nobs), metres */
  const float *obs;       /* obs(nobs) */
  const float *hdxb;      /* hdxb(nobs,0:k-1) */
} cwbl_radar_obs;

typedef struct cwbl_obs_set {
  int                   n_gts;
  int                   n_radar;
  const cwbl_gts_obs   *gts;     /* at most one entry per type id */
  const cwbl_radar_obs *radar;
  int                   memory;  /* CWBL_MEM_HOST / CWBL_MEM_DEVICE for the arrays */
  int                   reserved;
} cwbl_obs_set;

/* Namelist values of one obs type for the current variable (index ivar of the
 * per-variable arrays): gts_config / radar_variable_config, module_config.f90:7-34. */
typedef struct cwbl_type_params {
  int   use_it;                    /* %use_it */
  int   max_lz_pts;                /* %max_lz_pts */
  float hclr;                      /* %hclr(ivar) in km; <= 0 disables the type */
  float vclr;                      /* %vclr(ivar) in km; <= 0 = no vertical localization */
  float err_muti[CWBL_MAX_NVAR];   /* GTS: per obs variable %u..%q%err_muti; radar: [0] = %error */
  float err_rej[CWBL_MAX_NVAR];    /* GTS: per obs variable; radar: [0] = %err_rej */
  int   is_assim[CWBL_MAX_NVAR];   /* GTS: %u..%q%is_assim(ivar); radar: unused (hclr>0) */
} cwbl_type_params;

typedef struct cwbl_var_params {
  float multi_infl;      /* inflation_nml multi_infl(ivar): inflat=(k-1)/multi_infl (:68) */
  int   use_rtpp;
  float rtpp_alpha;
  int   use_rtps;
  float rtps_alpha;
  int   tune_q;          /* 1: letkf_tune_q (module_letkf_core.f90:702-733) on the analysed
                          * region after the analysis, as letkf_driver does for the Q
                          * species (QVAPOR ... QNHAIL, :253-278); Q3 (0/0 = NaN) replicated */
  cwbl_type_params gts[CWBL_NUM_GTS_TYPES];     /* index = gts type id - 1 */
  cwbl_type_params radar[CWBL_NUM_RADAR_TYPES]; /* index = radar type id - 1 */
} cwbl_var_params;

/* One variable's local slab, exactly as letkf_driver holds it (module_letkf_core.f90:85,
 * 171-172, 192-193): var(nx,ny,nz,0:k-1), lat/lon -> x/y(nx,ny), alt(alt_nx,alt_ny,nz). */
typedef struct cwbl_slab {
  int          nx, ny, nz;      /* leading dims of var and x/y */
  int          alt_nx, alt_ny;  /* leading dims of alt (cpu%loc_nx, cpu%loc_ny) */
  int          ix_lim, iy_lim;  /* analysed columns: i < ix_lim, j < iy_lim (:209-210, Q2) */
  int          memory;          /* CWBL_MEM_HOST / CWBL_MEM_DEVICE */
  const float *x;               /* proj%lonlat_to_xy(lon,lat)(1) per column, (nx,ny) */
  const float *y;               /* ... (2) */
  const float *alt;             /* alt(alt_nx,alt_ny,nz) metres */
  float       *var;             /* in/out var(nx,ny,nz,0:k-1) */
} cwbl_slab;

typedef struct cwbl_stats {
  long long points;          /* grid points visited (ix_lim*iy_lim*nz) */
  long long solved;          /* points with >= 1 accepted obs (letkf_solve called) */
  long long nobs_sum;        /* sum of p over solved points */
  long long lz_truncated;    /* (point, type) searches that hit max_lz_pts (Q4) */
  long long nonconverged;    /* Jacobi: eigensolves that hit the sweep cap (LAPACK info is */
                             /* ignored, module_eigen.f90:49); quadrature: points whose */
                             /* spectrum bound exceeds the last rule (max/min > 1e12) */
  long long q1_undefined;    /* (point, type) searches in the Q1 undefined case */
  long long sweeps_sum;      /* solver effort summed over solved points: Jacobi sweeps, or */
                             /* the quadrature rule's decade (default solver) */
  int       max_p;           /* max p over points */
  int       max_sweeps;      /* max of the same */
  int       ntrees;          /* trees built for this variable */
  int       reserved;
  double    ms_total;        /* wall time of the call */
  double    ms_prep;         /* tree build + obs QC tables; for a record-reuse candidate */
                             /* (equal key) also its slab staging and coordinate compare */
  double    ms_search;       /* neighbour search kernels */
  double    ms_solve;        /* solve kernels (+ the tune_q pass when requested) */
  double    ms_copy;         /* host<->device copies of the slab (host memory only; for a */
                             /* pageable slab: host time in its page-locked bounce copies). */
                             /* Piped transfers overlap the batches and are not counted, */
                             /* those of CWBL_OPT_HOST_PIPE = 1 included */
} cwbl_stats;

int         cwbl_init(const cwbl_init_params *params);
/* Device-memory calls (CWBL_MEM_DEVICE and the transpose helpers) are ordered after the work
 * queued so far on the caller's stream: an event recorded there, waited on by the library's
 * own streams.  `stream` is a hipStream_t (NULL = the legacy null stream, the default).  No
 * reference counterpart: the reference has no device (its arrays are complete on entry). */
int         cwbl_set_stream(void *stream);
int         cwbl_set_obs(const cwbl_obs_set *obs);
int         cwbl_analyze_var(const cwbl_var_params *vp, const cwbl_slab *slab,
                             cwbl_stats *stats /* nullable */);

/* cwbl_analyze_var for up to CWBL_MAX_GROUP_VARS variables that share a localisation, in one
 * call.  The LETKF weights of a grid point depend on the obs, the localisation, multi_infl and
 * the point's coordinates, not on the analysed variable.  Three paths fuse the group: on the
 * k = 17..40 record path the call searches, assembles and tridiagonalises once per point and
 * replays the factor on every variable (solve_tq40_multi_kernel); on the one-wavefront path
 * (k <= 16, k = 41..64, and k = 17..40 under CWBL_OPT_SPLIT40 = 0) a group of two or more
 * searches, assembles and tridiagonalises once per point with every variable carried through
 * the steps (solve_tq_multi_kernel); on the k = 65..128 hand-off path a group of two or more
 * does the same in the group forms of its kernel pair (solve_tq_big_multi_kernel or
 * solve_tq_rows_multi_kernel, then solve_tqb_tail_multi_kernel).  Each variable's result and
 * the counters are those of cwbl_analyze_var on the same inputs, bit for bit.  It keeps no
 * cache and neither reads, fills nor invalidates the record cache (CWBL_OPT_RECORD_REUSE), so
 * it saves the same work at any grid size and memory budget.  Elsewhere (CWBL_OPT_SOLVER = 1,
 * k > 64 under CWBL_OPT_BIG_PATH = 0, and a group of one outside the record path) the
 * variables run one after another through cwbl_analyze_var's code.
 *
 * Group rule (checked before any device work; a violation returns CWBL_ERR_ARG and the message
 * names the variable index and the field): 1 <= nvar <= CWBL_MAX_GROUP_VARS; every slabs[i]
 * equals slabs[0] in nx, ny, nz, alt_nx, alt_ny, ix_lim, iy_lim, memory and in the x, y, alt
 * POINTERS (the same arrays); the var ranges [var, var + nx ny nz k) are pairwise disjoint;
 * every vp[i] equals vp[0] in multi_infl and in all gts / radar type parameters.  use_rtpp,
 * rtpp_alpha, use_rtps, rtps_alpha and tune_q are free per variable.
 *
 * stats (nullable) is ONE struct: points of one slab; the counters are what cwbl_analyze_var
 * reports for any one variable of the group; the ms_* fields are the call's own times (summed
 * over the variables where they run one after another). */
#define CWBL_MAX_GROUP_VARS 8
int         cwbl_analyze_vars(int nvar, const cwbl_var_params *vp /* [nvar] */,
                              const cwbl_slab *slabs /* [nvar] */,
                              cwbl_stats *stats /* nullable, ONE */);

/* letkf_solve for npts points (module_letkf_core.f90:598-700).  Point i uses columns
 * [col_off[i], col_off[i+1]) of yo(ncol) and yb(k,ncol) (member fastest), xb(k,npts) ->
 * xa(k,npts).  evals (nullable) receives the eigenvalues of inflat*I + yb yb^T per point in
 * ascending order (k,npts), as dsyevd returns them in inverse_matrix (module_eigen.f90:48-49;
 * the reference keeps 1/lambda in eigen::eval afterwards), at every k <= 128. */
int         cwbl_solve_batch(int npts, const long long *col_off, const float *yo,
                             const float *yb, const float *xb, float inflat,
                             int use_rtpp, float rtpp_alpha, int use_rtps, float rtps_alpha,
                             float *xa, double *evals, int memory);

/* build_tree + get_lz for one obs type: obs_xyz(3,nobs) metres, hclr/vclr km
 * (vclr <= 0: 2-D), queries q_xyz(3,nq).  nfound(nq); idx/r2 (max_lz_pts,nq) in the
 * reference's traversal order (0-based obs indices). */
int         cwbl_search(int nobs, const float *obs_xyz, float hclr, float vclr,
                        int max_lz_pts, int nq, const float *q_xyz,
                        int *nfound, int *idx, float *r2, int memory);

/* ---- member <-> column transposes -----------------------------
 * The reference moves each variable between member layout (rank m holds member m's field
 * global(nx,ny,nz)) and column layout (each rank holds var(loc_nx,loc_ny,nz,0:k-1) for its
 * columns) with mpi_alltoallv (module_mpi_util.f90:190-358).  Columns are split cyclically,
 * block 1, over a px x py rank grid (letkf_local_info, :71-188; px >= py from
 * mpi_dims_create): rank r = id_x + id_y*px owns x = id_x + i*px, y = id_y + j*py (0-based).
 * The exchange itself is RCCL point-to-point (cwbl/transpose.py); these entry points do the
 * packing in device memory (all pointers are device pointers; px, py <= 64; each call has
 * completed when it returns). */

/* letkf_scatter_grid's send side (:224-258): global(nx,ny,nz) -> send, the rank-major
 * concatenation of global(xloc_r, yloc_r, :) for r = 0..px*py-1, each chunk
 * (loc_nx_r, loc_ny_r, nz) in Fortran order. */
int         cwbl_pack_columns(const float *global, int nx, int ny, int nz, int px, int py,
                              float *send);
/* letkf_gather_grid's receive side (:326-350): the inverse of cwbl_pack_columns. */
int         cwbl_unpack_columns(const float *recv, int nx, int ny, int nz, int px, int py,
                                float *global);
/* The same for nm member fields in one launch (the members a rank owns, k/N of them on an
 * N-GPU node): member i is global + i*gstride -> send + i*sstride (strides in elements, >= the
 * field's nx*ny*nz when nm > 1), and back. */
int         cwbl_pack_members(const float *global, long long gstride, int nm, int nx, int ny,
                              int nz, int px, int py, float *send, long long sstride);
int         cwbl_unpack_members(const float *recv, long long rstride, int nm, int nx, int ny,
                                int nz, int px, int py, float *global, long long gstride);
/* letkf_scatter_vcoord's reduction (:491-505): ph(n2d, nz_ph, 0:k-1), member slowest ->
 * alt(n2d, nz_out).  tmp = sgemv('n', n2d*nz_ph, k, 1.0/(g*k), ph, ., ones, 0.0) evaluated
 * in the reference BLAS order (y = 0; y += (alpha*1)*ph(:,m), m = 0..k-1, fp32); then
 * stagger 1: alt = tmp (nz_out = nz_ph); stagger 0: alt = (tmp(:,2:) + tmp(:,:nz_ph-1))*0.5
 * (nz_out = nz_ph - 1). */
int         cwbl_vcoord_mean(const float *ph, long long n2d, int nz_ph, int k, int stagger,
                             float g, float *alt);

/* ---- ensemble mean of the analysis (write_mean, module_grid.f90:700-840; SURVEY.md §8(f)
 * rank 4) ------------------------------------------------------------------------------------
 * The reference sums every analysed field over the member ranks with one mpi_reduce each
 * (:744-822) and scales the root's sums by nmember_inv with sscal (:827-...).  Here a rank
 * sums the members it holds (cwbl/transpose.py deals k/N members per rank), all fields packed
 * in one buffer; ONE RCCL reduce of that buffer follows, then the scale on the root.  Device
 * pointers; each call has completed when it returns. */
/* out(i) = sum over m = 0..nm-1 of fields(i, m), fp32, sequential in member order;
 * fields(n, nm) member slowest. */
int         cwbl_member_sum(const float *fields, long long n, int nm, float *out);
/* x(i) = alpha * x(i) (sscal, :827-...). */
int         cwbl_scale(float *x, long long n, float alpha);

/* ---- kernel timing (measurement; no reference counterpart) -------------------------------
 * With timing on, cwbl_analyze_var brackets every search and solve launch with a HIP event
 * pair on the stream the launch runs on and, after the call's final synchronisation, adds
 * the pair's elapsed time to that kernel's sum.  cwbl_set_kernel_timing(1) switches timing
 * on and clears the sums (0 switches it off); cwbl_kernel_times copies up to `cap` entries,
 * one per kernel launched since, and stores the number of such kernels in *n. */
typedef struct cwbl_kernel_time {
  char      name[64];   /* the kernel as rocprofv3 names it, template arguments included */
  long long launches;
  long long points;     /* grid points the launches processed (0: flagged-point re-search) */
  double    ms;         /* summed HIP-event time */
} cwbl_kernel_time;
int         cwbl_set_kernel_timing(int enable);
int         cwbl_kernel_times(cwbl_kernel_time *out, int cap, int *n);

/* ---- path options (no reference counterpart) ---------------------------------------------
 * The library reads no environment variable but OMP_NUM_THREADS (which caps the host threads
 * of the pageable-slab bounce fallback).  The alternative kernel paths and batch sizes below
 * are kept for A/B measurement and for the parity tests that compare one path with another;
 * they are set after cwbl_init, which resets every option to its default.  A value outside
 * an option's range returns CWBL_ERR_ARG.  No option changes a result beyond the fp64
 * summation order of the solve (every path meets the same parity bar). */
enum {
  CWBL_OPT_SOLVER = 1,         /* 0 Householder + quadrature (default); 1 the Jacobi
                                * eigensolver (k <= 64, analysis and solve_batch) */
  CWBL_OPT_SPLIT40 = 2,        /* k = 17..40: 1 assembly record + four-point solve (default);
                                * 0 the one-wavefront kernel */
  CWBL_OPT_SPLIT40_BATCH = 3,  /* points per record sub-batch of that path (0 = search batch) */
                               /* (4: the r4 two-stream record path, removed in r6: a tie) */
  CWBL_OPT_SEARCH = 5,         /* 0 uniform bins + tree for truncated lists (default); 1 the
                                * k-d tree walk for every point */
  CWBL_OPT_BIG_PATH = 6,       /* k = 65..128: 1 256-thread hand-off + one-wave tail (default);
                                * 0 one 256-thread kernel */
  CWBL_OPT_BIG_BATCH = 7,      /* points per k > 64 sub-batch (>= 64; default 98 304) */
  CWBL_OPT_PAGEABLE = 8,       /* pageable host slab: 0 page-lock in place (default); 1 bounce
                                * through the library's page-locked slots */
  CWBL_OPT_BIN_DIV = 9,        /* search bin side = radius / value, 1..8 (0 = by obs density);
                                * applies to the next cwbl_analyze_var (cached bins of another
                                * divisor are rebuilt) */
  CWBL_OPT_LEAD_DIV = 10,      /* first search batch = points / value (0 = off, default) */
  CWBL_OPT_MAX_BATCH = 11,     /* points per search batch, >= 256 (0 = automatic, default) */
  CWBL_OPT_INFO_WINDOW = 12,   /* points per reduction of the per-point solve info, >= 256
                                * (0 = 2^25, default; smaller values exercise the rollover) */
  CWBL_OPT_INDEX = 13,         /* search index of the next cwbl_analyze_var: 0 k-d tree and bins
                                * built on the host (default); 1 bins built on the device from
                                * the obs coordinates, columns in obs order, the k-d tree built
                                * by a host thread and used only where a list truncates (or
                                * for every point with CWBL_OPT_SEARCH = 1).  Cached indexes
                                * of the two modes are kept apart */
  CWBL_OPT_RECORD_REUSE = 14,  /* k = 17..40 record path: device memory budget in MiB for the
                                * assembled records kept from one cwbl_analyze_var to the next
                                * (0 = no reuse; default min(40 GiB, 40% of the device memory
                                * free at cwbl_init)).  A call whose obs set, options, type
                                * parameters, multi_infl, slab shape and coordinates equal the
                                * previous call's solves from the kept records and skips the
                                * QC columns, the search and the assembly: bit-identical
                                * results.  A budget below the slab's need keeps the leading
                                * batches that fit */
  CWBL_OPT_COLUMN_SHARE = 15,  /* cwbl_analyze_var of a variable whose used obs types all have
                                * vclr <= 0 (2-D localisation: the weights of a grid point then
                                * depend on its column only): 0 every point on its own (default);
                                * 1 one search, one assembly and one tridiagonalisation per
                                * column, every level solved from that factor: on the k = 17..40
                                * record path solve_tq40_column_kernel, on the one-wavefront and
                                * hand-off paths the group kernels over chunks of up to
                                * CWBL_MAX_GROUP_VARS levels; 2 the level-chunked group kernels on
                                * the record path too (the A/B partner of 1).  Equal counters.
                                * Results bit-identical to option 0 on the one-wavefront and
                                * hand-off paths; on the record path when ix_lim * iy_lim is a
                                * multiple of 4 or no wavefront of four points mixes quadrature
                                * round classes (see cwbl_column_info), otherwise equal within
                                * the parity bar.  A call that is not eligible (see
                                * cwbl_column_info) runs as under 0; a shared call runs with
                                * record reuse off (the cache is not read, filled or
                                * invalidated).  cwbl_analyze_vars with two or more variables
                                * ignores the option */
  CWBL_OPT_COLUMN_LEVELS = 16, /* levels per wavefront of solve_tq40_column_kernel, >= 1 (0 =
                                * automatic, default: all levels of the column unless the
                                * columns alone do not fill the device).  The result does not
                                * depend on it; tests use it to force level splits */
  CWBL_OPT_FACTOR_REUSE = 17,  /* what CWBL_OPT_RECORD_REUSE keeps of a point: 1 (default) the
                                * factor A = Q T Q^T of the record, written over its 6880 bytes
                                * by the call that fills the cache, and 640 bytes more with the
                                * reduction's step scalars, so a later call with an equal key
                                * skips the tridiagonalisation as well; 0 the assembled record
                                * itself, tridiagonalised again by every call.  Bit-identical
                                * results either way.  The budget bounds the 6880-byte part
                                * alone, so the cached batches, the key, the counters and
                                * cwbl_reuse_info's batch counts do not depend on it; its
                                * bytes_held includes the 640-byte part */
  CWBL_OPT_HIT_MERGE = 18,     /* a call that solves from the factor cache (a hit under
                                * CWBL_OPT_FACTOR_REUSE: one variable, slab resident or staged
                                * whole) issues 1 (default) one launch per info window for all
                                * its cached batches, 0 one launch per cached batch.
                                * Bit-identical results either way.  Nothing that is cached
                                * depends on it: setting it leaves a filled cache valid */
  CWBL_OPT_WAVE_REUSE = 19,    /* 1: cwbl_analyze_var on the one-wavefront path at k = 41..64
                                * (default solver) keeps each point's factor A = Q T Q^T for the
                                * next call, within the CWBL_OPT_RECORD_REUSE budget (0 there
                                * turns this cache off too): KP (KP - 1) / 2 + 5 KP fp64 words per
                                * point at KP = 48, 56, 64 (10.9, 14.6, 18.7 KB).  A later call
                                * with an equal key (the record cache's, and KP) and bit-equal
                                * coordinates runs no obs preparation, search, assembly or
                                * tridiagonalisation: one solve_tq_wave_factor_kernel per cached
                                * batch.  Bit-identical results and equal counters; reported
                                * through cwbl_reuse_info like the record cache.  0 (default):
                                * nothing is kept and the path runs as without the option.
                                * Accepted and ignored at k <= 16 and at k = 17..40 under
                                * CWBL_OPT_SPLIT40 = 0.  Group calls and column-shared calls
                                * neither read, fill nor invalidate the cache */
  CWBL_OPT_HOST_PIPE = 20,     /* host-memory slabs (CWBL_MEM_HOST) of the calls that otherwise
                                * move var whole around the batches.  1: a group call
                                * (cwbl_analyze_vars on a fused path) and a column-shared call
                                * pipe var batch by batch as cwbl_analyze_var does, each
                                * pageable var page-locked in place for the call; and a piped
                                * call with tune_q = 1 (single calls included, through the
                                * bounce slots too) runs tune_q_kernel over each batch right
                                * behind its solve, so its analysis comes back batch by batch
                                * as well.  A call still moves whole when the analysed region
                                * is not the whole horizontal slab, when a registration fails,
                                * or when CWBL_OPT_PAGEABLE = 1 meets a pageable var of a group
                                * or a column-shared call (cwbl_transfer_info names the case).
                                * 0 (default): every call moves its slab as without the
                                * option.  Bit-identical results and equal counters either
                                * way.  Nothing that is cached depends on it: setting it leaves
                                * a filled cache valid */
  CWBL_OPT_BIG_REUSE = 21,     /* 1: cwbl_analyze_var on the hand-off path at k = 65..96 (KP = 96,
                                * default solver, CWBL_OPT_BIG_PATH = 1) keeps each point's
                                * factor A = Q T Q^T for the next call, within the
                                * CWBL_OPT_RECORD_REUSE budget (0 there turns this cache off
                                * too): at most KP (KP - 1) / 2 + 5 KP fp64 words per point
                                * (4977 words, 39.8 KB).  A later call with an equal key (the
                                * record cache's, and KP) and bit-equal coordinates runs no obs
                                * preparation, search, assembly, hand-off kernel or
                                * tridiagonalisation: one solve_tqb_factor_kernel per cached
                                * sub-batch (CWBL_OPT_BIG_BATCH).  Bit-identical results and
                                * equal counters; reported through cwbl_reuse_info like the
                                * record cache.  0 (default): nothing is kept and the path runs
                                * as without the option; setting 0 releases what is held.
                                * Accepted and ignored at k = 97..128 and on every other path
                                * (k <= 64, CWBL_OPT_BIG_PATH = 0).  Group calls and
                                * column-shared calls neither read, fill nor invalidate the
                                * cache */
  CWBL_OPT_ROWS_REUSE = 22,    /* 1: cwbl_analyze_var on the hand-off path at k = 97..128
                                * (KP = 128, default solver, CWBL_OPT_BIG_PATH = 1) keeps each
                                * point's factor A = Q T Q^T for the next call, as
                                * CWBL_OPT_BIG_REUSE does at KP = 96 and within the same
                                * CWBL_OPT_RECORD_REUSE budget (0 there turns this cache off
                                * too): at most KP (KP - 1) / 2 + 5 KP fp64 words per point
                                * (8705 words, 69.6 KB).  A later call with an equal key and
                                * bit-equal coordinates runs no obs preparation, search,
                                * assembly, hand-off kernel or tridiagonalisation: one
                                * solve_tqb_factor_kernel per cached sub-batch
                                * (CWBL_OPT_BIG_BATCH).  Bit-identical results and equal
                                * counters; reported through cwbl_reuse_info.  0 (default):
                                * nothing is kept and the path runs as without the option;
                                * setting 0 releases what is held.  Accepted and ignored at
                                * k <= 96 and under CWBL_OPT_BIG_PATH = 0.  Group calls and
                                * column-shared calls neither read, fill nor invalidate the
                                * cache */
  CWBL_OPT_COLUMN_FACTOR = 23, /* 1: a call that is shared per column (CWBL_OPT_COLUMN_SHARE 1
                                * or 2, eligible as there) on the one-wavefront path at
                                * k = 41..64 or on the hand-off path at k = 65..96 solves every
                                * level from one kept factor per column instead of running the
                                * levels as group launches of eight.  Per (sub-)batch of
                                * columns the factor cache's fill kernel analyses level 0 and
                                * leaves each column's factor A = Q T Q^T (the WaveFactor or
                                * BigFactor of CWBL_OPT_WAVE_REUSE and CWBL_OPT_BIG_REUSE) in a
                                * workspace of the call, and one launch of
                                * solve_tq_wave_factor_column_kernel<KP> or
                                * solve_tqb_factor_column_kernel<96, 32> solves the levels
                                * 1 .. nz-1 from it, CWBL_OPT_COLUMN_LEVELS levels per wavefront
                                * (0: automatic).  Bit-identical results and equal counters,
                                * whatever the level split.  The workspace is a grow-only device
                                * buffer of one (sub-)batch's factors (KP (KP - 1) / 2 + 5 KP
                                * fp64 words per column at most); nothing is kept between
                                * calls, and the record cache is neither read, filled nor
                                * invalidated.  If the workspace cannot be allocated the call
                                * runs the level chunks; that is no error.  0 (default): the
                                * shared call runs as without the option and no memory is
                                * taken.  Accepted and ignored everywhere else: k <= 40,
                                * k = 97..128, CWBL_OPT_SOLVER = 1, CWBL_OPT_BIG_PATH = 0, group
                                * calls and calls that are not shared.  Nothing that is cached
                                * depends on it: setting it leaves a filled cache valid.  With
                                * CWBL_OPT_COLUMN_ROWS = 1 the hand-off path at KP = 128 is served
                                * as well, as at KP = 96: fill_tqb_tail_kernel<128, 64> and
                                * solve_tqb_factor_column_kernel<128, 64> */
  CWBL_OPT_COLUMN_REUSE = 24,  /* device-memory budget in MiB of the column cache: what a call
                                * that is shared per column keeps for the next one (0 = off, the
                                * default; 0 releases what is held; cwbl_init resets it).  The
                                * weights of such a call depend on the column (i, j) alone, not
                                * on nz, the levels or alt, so the variables of one localisation
                                * whose slabs share x and y (MU, P, PH: nz = 1, nz, nz + 1) pay one
                                * search, assembly and reduction.  Eligible: a call that is shared
                                * under CWBL_OPT_COLUMN_SHARE 1 or 2 (see cwbl_column_info), and
                                * with this option on also a call of one variable with nz = 1 that
                                * meets every other condition there; it runs on the column view
                                * with one level (cwbl_column_info: shared = 1, levels = 1), bit
                                * for bit the per-point call.  Kept per column of the leading
                                * column batches that fit the budget: on the record path
                                * (k = 17..40) the assembled record (6880 B), on the one-wavefront
                                * path at k = 41..64 and the hand-off path at k = 65..96 the
                                * factor A = Q T Q^T that CWBL_OPT_COLUMN_FACTOR's fill leaves
                                * (KP (KP - 1) / 2 + 5 KP fp64 words at most), with the accepted
                                * counts and a snapshot of x and y.  Cached batches always run
                                * the one-factor form, whatever CWBL_OPT_COLUMN_SHARE (1 or 2) and
                                * CWBL_OPT_COLUMN_FACTOR say; batches beyond the budget run what
                                * they run without the option.  A later eligible call hits when
                                * the obs set, the options, KP, multi_infl, the types' parameters,
                                * nx, ny, ix_lim, iy_lim and the batch plan are equal and x and y
                                * equal the snapshot bit for bit (nz, alt, RTPP / RTPS, tune_q and
                                * the memory kind may differ).  A hit runs no obs preparation,
                                * search, assembly, hand-off kernel or fill for the cached
                                * batches: one launch per cached (sub-)batch solves all nz levels
                                * (solve_tq40_column_kernel on the kept records;
                                * solve_tq_wave_factor_column_all_kernel<KP> or
                                * solve_tqb_factor_column_all_kernel<96, 32> on the kept factors).
                                * Bit-identical results and equal counters; cwbl_column_reuse_info
                                * reports.  Anything else is a miss and refills.  A failed
                                * allocation is no error: the call runs without the cache.  The
                                * record cache (CWBL_OPT_RECORD_REUSE) is neither read, filled nor
                                * invalidated by a column call, and a per-point call never touches
                                * the column cache.  Accepted and ignored at k <= 16, k = 97..128,
                                * CWBL_OPT_SPLIT40 = 0, CWBL_OPT_SOLVER = 1, CWBL_OPT_BIG_PATH = 0
                                * and for group calls.  With CWBL_OPT_COLUMN_ROWS = 1 the hand-off
                                * path at KP = 128 is served as well, as at KP = 96: the kept
                                * factor is the BigFactor<128, 64> (8705 words, 69.6 KB per column)
                                * and a hit runs solve_tqb_factor_column_all_kernel<128, 64> */
  CWBL_OPT_COLUMN_ROWS = 25,   /* 1: the hand-off path at KP = 128 (the ensemble sizes above 96
                                * up to 128, default solver, CWBL_OPT_BIG_PATH = 1) becomes
                                * eligible for CWBL_OPT_COLUMN_FACTOR and CWBL_OPT_COLUMN_REUSE,
                                * which then hold there as they hold at KP = 96: the fill of
                                * CWBL_OPT_ROWS_REUSE (fill_tqb_tail_kernel<128, 64> behind the
                                * half-row hand-off kernel) analyses level 0 and leaves one
                                * factor per column, and solve_tqb_factor_column_kernel<128, 64>
                                * (a column-cache hit: solve_tqb_factor_column_all_kernel
                                * <128, 64>) solves the levels from it instead of the level
                                * chunks, which repeat the assembly and the reduction every eight
                                * levels.  Bit-identical results and equal counters.  It does
                                * nothing on its own: the two options still have to be set.  The
                                * workspace of CWBL_OPT_COLUMN_FACTOR is 69.6 KB per column of a
                                * sub-batch (CWBL_OPT_BIG_BATCH; 6.8 GB at its default); a failed
                                * allocation still means the level chunks and no error.  The
                                * per-point cache of CWBL_OPT_ROWS_REUSE is neither read, filled
                                * nor invalidated by a column call.  0 (default; cwbl_init resets
                                * it): every call launches what it launches without the option;
                                * setting 0 releases what the two options hold at KP = 128.
                                * Accepted and ignored at the ensemble sizes up to 96, under
                                * CWBL_OPT_BIG_PATH = 0, under CWBL_OPT_SOLVER = 1 and for group
                                * calls.  Setting it starts a new generation of both caches */
  CWBL_OPT_INDEX_ORDER = 26    /* how CWBL_OPT_INDEX = 1 numbers an obs type's columns.  0
                                * (default; cwbl_init resets it): a column's slot is its obs
                                * index, and every call launches what it launches without the
                                * option.  1: the slot is the position in the cell-sorted order of
                                * the type's bins (cwbl_bin_index's `order`), so the columns of one
                                * neighbourhood lie close together, as they do in the k-d tree's
                                * slot order of CWBL_OPT_INDEX = 0.  Per type the library then
                                * keeps the sorted obs indices and their inverse (4 bytes per obs
                                * each) and, for a type whose tree is walked, the tree's slots as
                                * positions (4 bytes per obs); the solve reads its coordinates
                                * from the bins' own points, the columns are gathered through the
                                * sorted obs indices.  The neighbour lists keep their order (the
                                * cells visited, ascending obs index within a cell, kdtree2's
                                * order where a list truncates): only the labels change, so
                                * results are bit-identical to 0 with equal counters.  A changed
                                * CWBL_OPT_BIN_DIV rebuilds the bins and the numbering and keeps
                                * the tree.  Accepted and ignored under CWBL_OPT_INDEX = 0.
                                * Setting it starts a new generation of both caches; see
                                * cwbl_index_info and cwbl_index_slots */
};
int         cwbl_set_option(int option, long long value);

/* ---- search index (no reference counterpart: the reference walks its k-d tree) ------------
 * The uniform bins of the analysis search for one obs type, built on the device: the
 * counterpart of cwbl_search for the binned path.  obs_xyz(3,nobs) metres, hclr/vclr km
 * (vclr <= 0: 2-D); div: cell side = search radius / div, 1..8 (0 = by obs density).  The
 * grid is that of the analysis: origin at the minima of the finite normalised coordinates,
 * cell (ix, iy, iz) = floor((x - x0) * binv) per dimension clamped to the grid (fp32), cells
 * x-fastest, a point with a non-finite coordinate in cell 0.  order(nobs): the obs indices
 * (0-based) sorted by cell, ascending within a cell; start(ncell + 1): cell c holds
 * order[start[c] .. start[c + 1]).  With start == NULL only `grid` is filled, so the caller
 * can size start (nbx*nby*nbz + 1 entries, start_cap says how many it holds) and order.
 * `memory` tells where obs_xyz, start and order live. */
typedef struct cwbl_bin_grid {
  float x0, y0, z0, binv;   /* origin and 1 / cell side, normalised units */
  int   nbx, nby, nbz;      /* cells per dimension (nbz = 1 in 2-D); at most 2^22 in all */
  int   div;                /* the divisor used (the cap may have grown the cells beyond it) */
} cwbl_bin_grid;
int         cwbl_bin_index(int nobs, const float *obs_xyz, float hclr, float vclr, int div,
                           cwbl_bin_grid *grid, long long start_cap, int *start, int *order,
                           int memory);

/* What the last cwbl_analyze_var spent on its search index (the split of cwbl_stats.ms_prep),
 * in both index modes. */
typedef struct cwbl_prep_info_t {
  int    trees_built;      /* host k-d tree builds started by the call */
  int    bins_built;       /* bin sets built by the call (0: all came from the cache) */
  int    bins_on_device;   /* of those, built on the device */
  int    flagged_batches;  /* CWBL_OPT_INDEX = 1: search batches with a point whose list
                            * passes max_lz_pts (mode 0 never reads the count back) */
  double ms_tree;          /* host time of the k-d builds the call used (CWBL_OPT_INDEX = 1:
                            * the worker's own time, counted when the tree is first needed) */
  double ms_bins;          /* host build_bins, or the device build on its stream (HIP events) */
  double ms_columns;       /* obs_prep_kernel (HIP events) */
  double ms_tree_wait;     /* CWBL_OPT_INDEX = 1: time the call waited for a tree worker */
} cwbl_prep_info_t;
int         cwbl_prep_info(cwbl_prep_info_t *out);

/* How the last cwbl_analyze_var numbered the columns of its obs types (a call served entirely
 * from the record or column cache plans no index and reports types = 0). */
typedef struct cwbl_index_info_t {
  int index_mode;      /* CWBL_OPT_INDEX of the call */
  int cell_order;      /* 1: every obs type of the call was numbered in the cell order of its
                        * bins (CWBL_OPT_INDEX = 1 with CWBL_OPT_INDEX_ORDER = 1) */
  int types;           /* obs types the call searched */
  int trees_composed;  /* k-d trees whose slots the call rewrote as cell-order positions: a tree
                        * first needed by a search, or one already up when the bins changed */
} cwbl_index_info_t;
int         cwbl_index_info(cwbl_index_info_t *out);
/* The slot -> obs index (0-based) table the last cwbl_analyze_var used for one obs type
 * (family 0 GTS, 1 radar; type_id as in cwbl_obs_set), copied to host memory: the k-d tree's
 * permutation under CWBL_OPT_INDEX = 0, the identity under CWBL_OPT_INDEX = 1, and
 * cwbl_bin_index's `order` under CWBL_OPT_INDEX = 1 with CWBL_OPT_INDEX_ORDER = 1.  *n is the
 * type's obs count; min(cap, *n) entries of slot_obs are written.  CWBL_ERR_STATE before the
 * first cwbl_analyze_var, CWBL_ERR_ARG for a type the call did not use. */
int         cwbl_index_slots(int family, int type_id, int cap, int *slot_obs, int *n);

/* What the last cwbl_analyze_var reused (CWBL_OPT_RECORD_REUSE). */
typedef struct cwbl_reuse_info_t {
  long long batches_reused;     /* search batches solved from kept records */
  long long batches_assembled;  /* search batches that ran the search and the assembly */
  long long bytes_held;         /* device memory of the cache: records (or factors and their
                                 * step scalars), accepted counts and the coordinate snapshot */
  double    ms_compare;         /* host time of the coordinate compare, its read-back and
                                 * synchronisation included (0: the key already differed) */
} cwbl_reuse_info_t;
int         cwbl_reuse_info(cwbl_reuse_info_t *out);

/* What the last cwbl_analyze_var (or cwbl_analyze_vars) did under CWBL_OPT_COLUMN_SHARE.
 *
 * Bit identity with option 0.  The one-wavefront and hand-off kernels solve one point per
 * wavefront, and a shared call's result there equals option 0's bit for bit.  The record
 * path's kernels solve four points per wavefront, and the wavefront runs the quadrature rule
 * of the largest round class (15, 23, 31 or 63 nodes: spectrum bound M/m up to 1e3, 1e5, 1e12,
 * beyond) among its four points.  Option 0 puts the points g = 4n .. 4n + 3 of the slab
 * (g = i + ix_lim (j + iy_lim kz)) in a wavefront, a shared call the columns 4n .. 4n + 3 at
 * every level.  The two groupings are the same when ix_lim * iy_lim is a multiple of 4; then,
 * or whenever no wavefront of either grouping mixes round classes, the results are equal bit
 * for bit.  Otherwise a point of a lower class may run a longer rule under one option than
 * under the other: both results meet the parity bar (the rules agree to ~1e-12 relative, far
 * below the fp32 rounding of the analysis), the low bits of some values differ.  Options 1 and
 * 2 always agree with each other bit for bit, whatever CWBL_OPT_COLUMN_LEVELS.
 *
 * Eligibility.  A call is shared when the option is non-zero, it analyses one variable, nz >= 2
 * (nz = 1 as well where CWBL_OPT_COLUMN_REUSE is on and applies), the default
 * solver runs on the record, the one-wavefront or the hand-off path, and every tree of the
 * call is 2-D with a 2-D query and outside the Q1 undefined case; the check is made after the
 * trees are planned, before any batch work. */
enum {
  CWBL_COLUMN_SHARED = 0,         /* shared (reason of a shared call) */
  CWBL_COLUMN_REASON_OFF = 1,     /* the option is 0 */
  CWBL_COLUMN_REASON_3D = 2,      /* a used obs type has vclr > 0 */
  CWBL_COLUMN_REASON_Q1 = 3,      /* a family in the Q1 undefined case (CWBL_Q1_REPLICATE) */
  CWBL_COLUMN_REASON_NZ = 4,      /* nz < 2 (nz < 1 where CWBL_OPT_COLUMN_REUSE applies) */
  CWBL_COLUMN_REASON_PATH = 5,    /* CWBL_OPT_SOLVER = 1, or k > 64 under CWBL_OPT_BIG_PATH = 0 */
  CWBL_COLUMN_REASON_GROUP = 6,   /* cwbl_analyze_vars with two or more variables */
  CWBL_COLUMN_REASON_NO_TREES = 7 /* nothing to assimilate: no tree, no analysis */
};
typedef struct cwbl_column_info_t {
  int       shared;           /* 1: the call ran once per column */
  int       reason;           /* CWBL_COLUMN_REASON_* when not shared, else CWBL_COLUMN_SHARED */
  long long columns;          /* ix_lim * iy_lim (0 when not shared) */
  int       levels;           /* nz (0 when not shared) */
  int       levels_per_wave;  /* solve_tq40_column_kernel, or the level kernel of
                               * CWBL_OPT_COLUMN_FACTOR (over the levels 1 .. nz-1): levels per
                               * wavefront of the last launch; 0 on the chunked paths */
  int       chunk_launches;   /* chunked paths: launches per (sub-)batch, one per chunk of up
                               * to CWBL_MAX_GROUP_VARS levels (a remainder of one level runs
                               * the single kernel and counts); 0 for the column kernel and
                               * when from_factor is 1 */
  int       from_factor;      /* 1: the levels were solved from one kept factor per column
                               * (CWBL_OPT_COLUMN_FACTOR) */
} cwbl_column_info_t;
int         cwbl_column_info(cwbl_column_info_t *out);

/* What the last cwbl_analyze_var did with the column cache (CWBL_OPT_COLUMN_REUSE).  A call that
 * is not eligible, or runs with the option off, reports zeros but bytes_held. */
enum {
  CWBL_COLUMN_FORM_NONE = 0,     /* nothing kept */
  CWBL_COLUMN_FORM_RECORDS = 1,  /* AsmRecord<40> per column (k = 17..40) */
  CWBL_COLUMN_FORM_WAVE = 2,     /* WaveFactor<KP> per column (k = 41..64) */
  CWBL_COLUMN_FORM_BIG = 3       /* BigFactor<96, 32> per column (k = 65..96) */
};
typedef struct cwbl_column_reuse_info_t {
  long long columns_reused;   /* columns whose levels were solved from what an earlier call kept */
  long long columns_filled;   /* columns whose record or factor this call left in the cache */
  long long batches_reused;   /* column batches solved from the cache */
  long long bytes_held;       /* device memory of the column cache after the call: records or
                               * factors, accepted counts and the snapshot of x and y */
  double    ms_compare;       /* host time of the compare of x and y with the snapshot, its
                               * read-back and synchronisation included (0: the key differed) */
  int       form;             /* CWBL_COLUMN_FORM_* of what the cache holds after the call */
  int       reserved;         /* 0 */
} cwbl_column_reuse_info_t;
int         cwbl_column_reuse_info(cwbl_column_reuse_info_t *out);

/* How the last cwbl_analyze_var (or cwbl_analyze_vars) moved its slab's var between host and
 * device.  A CWBL_MEM_DEVICE call reports zeros.  The bytes are var's alone (x, y and alt are
 * staged before the batches in every mode), summed over the variables of a group.  Where the
 * variables of cwbl_analyze_vars run one after another, this is the last variable's call. */
enum {
  CWBL_TRANSFER_PIPED = 0,           /* nothing moved whole (also: device slab, nothing to do) */
  CWBL_TRANSFER_REASON_OFF = 1,      /* CWBL_OPT_HOST_PIPE is 0: a group or column-shared call
                                      * moved whole both ways, a single call with tune_q = 1
                                      * came back whole */
  CWBL_TRANSFER_REASON_REGION = 2,   /* ix_lim < nx or iy_lim < ny: a batch is no contiguous run */
  CWBL_TRANSFER_REASON_REGISTER = 3, /* a group or column-shared call: hipHostRegister failed
                                      * for a var (a locked-memory limit, for instance) */
  CWBL_TRANSFER_REASON_BOUNCE = 4    /* CWBL_OPT_PAGEABLE = 1 with a pageable var of a group or
                                      * column-shared call: those have no bounce-slot mode */
};
typedef struct cwbl_transfer_info_t {
  int       host;             /* 1: the slab was CWBL_MEM_HOST */
  int       piped;            /* 1: var went up batch by batch (S.h2d under the solves) */
  int       piped_back;       /* 1: the analysis came back batch by batch */
  int       registered;       /* var arrays page-locked in place for the call */
  int       bounce;           /* 1: through the library's page-locked bounce slots */
  int       reason;           /* CWBL_TRANSFER_REASON_* when a direction moved whole */
  long long tune_q_launches;  /* tune_q_kernel launches: one per flagged variable, or one per
                               * batch and flagged variable when the call tuned per batch */
  long long bytes_piped_up;   /* var bytes moved batch by batch, host to device */
  long long bytes_piped_down; /* ... and device to host */
  long long bytes_whole_up;   /* var bytes moved before the first batch */
  long long bytes_whole_down; /* ... and after the last */
} cwbl_transfer_info_t;
int         cwbl_transfer_info(cwbl_transfer_info_t *out);

int         cwbl_finalize(void);
const char *cwbl_last_error(void);
int         cwbl_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CWB_LETKF_CORE_H */
