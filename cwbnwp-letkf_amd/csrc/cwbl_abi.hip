// cwbl_abi.hip — C ABI of the LETKF analysis core (include/cwb_letkf_core.h).
//
// Host orchestration of one variable, mirroring letkf_driver (module_letkf_core.f90:59-297):
//   build_tree x2        -> host kdtree2-compatible build, upload (kdtree_build.cpp)
//   (point-independent)  -> obs_prep_kernel per obs type (QC / mean / spread columns)
//   points :209-240      -> batches of {search_kernel, solve_kernel<KP>} on one HIP stream
// The library owns its device buffers between cwbl_set_obs and cwbl_finalize; host arrays
// handed in are copied inside the call.  There is no CPU fallback: without a gfx950 device
// every compute entry point fails with CWBL_ERR_NO_DEVICE.
#include "../../include/cwb_letkf_core.h"
#include "cwbl_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace cwbl {
namespace {

std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(CWBL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                  __FILE__, __LINE__);                                                     \
  } while (0)

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) n = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

// grow-only page-locked host buffer (bounce slots of pageable host slabs)
struct PinBuf {
  void *p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e == hipSuccess) n = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

// A few persistent host threads for the bounce copies: run(n, fn) calls fn(0..n-1) spread
// over the threads and the caller, and returns when all calls are done.
class HostPool {
 public:
  ~HostPool() { stop(); }
  void run(int n, const std::function<void(int)> &fn) {
    if (n <= 0) return;
    start();
    {
      std::unique_lock<std::mutex> lk(mu_);
      fn_ = &fn;
      n_ = n;
      next_ = 0;
      busy_ = (int)th_.size();
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return busy_ == 0; });
    fn_ = nullptr;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (auto &t : th_) t.join();
    th_.clear();
    quit_ = false;
  }

 private:
  void start() {
    if (!th_.empty()) return;
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    int nt = (int)std::min(15u, hw - 1);  // + the calling thread: at most 16
    if (const char *e = std::getenv("OMP_NUM_THREADS"))
      nt = std::max(0, std::min(nt, std::atoi(e) - 1));
    // a new worker starts at the current generation: stop() of an earlier pool raised gen_,
    // and a worker starting from 0 would run a pass no run() handed out (and decrement
    // busy_ twice)
    unsigned long g;
    {
      std::lock_guard<std::mutex> lk(mu_);
      g = gen_;
    }
    for (int i = 0; i < nt; ++i) th_.emplace_back([this, g] { loop(g); });
  }
  void work() {
    for (;;) {
      int i;
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (!fn_ || next_ >= n_) return;
        i = next_++;
      }
      (*fn_)(i);
    }
  }
  void loop(unsigned long seen) {
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (quit_) return;
      }
      work();
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (--busy_ == 0) done_.notify_all();
      }
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int)> *fn_ = nullptr;
  int n_ = 0, next_ = 0, busy_ = 0;
  unsigned long gen_ = 0;
  bool quit_ = false;
};

struct ObsType {
  int family = 0, type_id = 0, nvar = 1, nobs = 0;
  std::vector<float> xyz;   // host copy (3,nobs) for tree builds
  DevBuf obs, error, hdxb, qc;
  DevBuf dxyz;              // xyz on the device, uploaded by the first device bin build
  bool dxyz_ok = false;
};

// One k-d tree of an obs type and its column tables.  The tree depends only on the obs
// coordinates and the normalisation (hclr, vclr, dimension), so it is kept across
// cwbl_analyze_var calls of one obs set; the column tables are rebuilt per call (they
// depend on the variable's QC parameters).
struct TreeBufs {
  int entry = -1, dim = 0, depth = 0;
  int bin_div_opt = 0;  // CWBL_OPT_BIN_DIV the bins were built under
  float hinv = 0.0f, vinv = 0.0f;
  DevBuf nodes, rdata, ind, col_bg, col_omm, col_err, col_ok;
  DevBuf bxyz, bstart;  // uniform bins of the same coordinates (search_binned_kernel)
  HostTree host;
  HostBins bins;
  // CWBL_OPT_INDEX = 1: the bins come from the device (ncoord: the normalised coordinates in
  // obs order, which are also the solve's rdata), the tree from a host worker thread that is
  // joined when a search first needs the tree (tree_ready: built, checked and uploaded)
  int mode = 0;
  int n = 0, bin_div_used = 0;
  DevBuf ncoord;
  IndexBounds bounds{};
  std::thread worker;
  bool worker_started = false, worker_joined = false, tree_ready = false;
  double worker_ms = 0.0;
  // CWBL_OPT_INDEX_ORDER = 1 (cell_order): a slot is the position in the bins' cell-sorted
  // order.  order[p]: the obs index at position p (the columns' slot_obs); rank: its inverse;
  // ind2[i] = rank[ind[i]]: the tree's slots as positions, composed once the tree is up.  The
  // solve reads its coordinates from bxyz, whose payload is then p.
  int cell_order = 0;
  DevBuf order, rank, ind2;
  void join() {
    if (worker.joinable()) worker.join();
    worker_joined = worker_started;
  }
  void release() {
    join();
    nodes.release(); rdata.release(); ind.release(); col_bg.release();
    col_omm.release(); col_err.release(); col_ok.release(); bxyz.release(); bstart.release();
    ncoord.release(); order.release(); rank.release(); ind2.release();
  }
  ~TreeBufs() { join(); }
};

enum KernelId {
  KT_SEARCH_BINNED, KT_SEARCH_FLAGGED, KT_SEARCH_TREE, KT_ASSEMBLE_RECORD, KT_SOLVE_TQ40,
  KT_SOLVE_TQ40_MULTI, KT_SOLVE_TQ40_COLUMN, KT_FILL_TQ40_FACTOR, KT_SOLVE_TQ40_FACTOR, KT_SOLVE_TQ_MULTI2, KT_SOLVE_TQ_MULTI4, KT_SOLVE_TQ_MULTI8,
  KT_BIG_HANDOFF, KT_TQB_TAIL, KT_FILL_TQB_TAIL, KT_SOLVE_TQB_FACTOR, KT_BIG_HANDOFF_MULTI2, KT_BIG_HANDOFF_MULTI4,
  KT_BIG_HANDOFF_MULTI8, KT_TQB_TAIL_MULTI2, KT_TQB_TAIL_MULTI4, KT_TQB_TAIL_MULTI8,
  KT_SOLVE_TQ, KT_FILL_TQ_WAVE, KT_SOLVE_TQ_WAVE_FACTOR, KT_SOLVE_TQ_BIG, KT_SOLVE_JACOBI,
  KT_TUNE_Q, KT_SOLVE_TQ_WAVE_FACTOR_COLUMN, KT_SOLVE_TQB_FACTOR_COLUMN,
  KT_SOLVE_TQ_WAVE_FACTOR_COLUMN_ALL, KT_SOLVE_TQB_FACTOR_COLUMN_ALL,
  KT_COUNT
};
struct KTime { long long launches = 0, points = 0; double ms = 0.0; };

// Record reuse (CWBL_OPT_RECORD_REUSE): a single-variable call keeps what its leading batches
// computed before the analysed variable enters: functions of the obs set, the types' parameters,
// the weight function, multi_infl and the point coordinates, which the key and a coordinate
// snapshot cover.  A later call with an equal key and bit-equal coordinates (a hit) launches
// the hit kernel on what was kept and nothing before it.  What is kept per point is the form:
//   form        path (call_form)              a cached point      a fill's solve; a hit
//   Records     k = 17..40, FACTOR_REUSE = 0  AsmRecord<40>       solve_tq40_kernel; the same
//   Tq40Factor  k = 17..40, FACTOR_REUSE = 1  FactorRecord<40>    fill_tq40_factor_kernel;
//                                             in its words        solve_tq40_factor_kernel
//   WaveFactor  k = 41..64, WAVE_REUSE        WaveFactor<KP>      fill_tq_wave_kernel;
//                                                                 solve_tq_wave_factor_kernel
//   BigFactor   k = 65..96, BIG_REUSE         BigFactor<96, 32>   fill_tqb_tail_kernel behind the
//               k = 97..128, ROWS_REUSE       BigFactor<128, 64>  hand-off kernel;
//                                                                 solve_tqb_factor_kernel
// The budget bounds the points' words.  Tq40Factor alone keeps more: beta and tau of the steps,
// a FactorAux entry per record outside the budget, so what is cached does not depend on
// FACTOR_REUSE.  The cached form and the live options cannot disagree on a hit: the key holds
// State::gen and KP, and cwbl_set_option bumps gen for every option that call_form reads.
//
// The column cache (CWBL_OPT_COLUMN_REUSE): what a column-shared call keeps per COLUMN of its
// leading column batches, for the next shared call of the same localisation on the same x and y,
// whatever its nz, alt and epilogue flags (MU, P, PH).  The record cache is per point and a
// column call never touches it; a per-point call never touches the column cache.
//   form        path (column_form)         a cached column      a fill; a hit
//   Records     k = 17..40                 AsmRecord<40>        assemble_record_kernel into the
//                                                               region, solve_tq40_column_kernel;
//                                                               the latter alone
//   WaveFactor  k = 41..64                 WaveFactor<KP>       fill_tq_wave_kernel (level 0) and
//                                                               the level kernel from level 1;
//                                                               the all-levels kernel
//   BigFactor   k = 65..96                 BigFactor<96, 32>    the hand-off kernel,
//               k = 97..128, COLUMN_ROWS   BigFactor<128, 64>   fill_tqb_tail_kernel and the level
//                                                               kernel from level 1; the
//                                                               all-levels kernel
// Its key holds 0 for nz, alt_nx and alt_ny, and its snapshot no alt: a 2-D tree reads neither
// the level nor alt.
//
// Both are one Cache, filled and read by one text (cache_candidate, cache_coords_match,
// begin_cache_fill, complete_cache_call); where they differ, per_column (of the call that is
// bound to one: v.colcache) says so there.
enum class CacheForm { None, Records, Tq40Factor, WaveFactor, BigFactor };
size_t form_words(CacheForm f, int kp) {  // fp64 words per cached point
  return f == CacheForm::WaveFactor  ? wave_factor_words(kp)
         : f == CacheForm::BigFactor ? big_factor_words(kp)
                                     : (size_t)AsmRecord<kTq4KP>::WORDS;
}
bool form_has_aux(CacheForm f) { return f == CacheForm::Tq40Factor; }  // a FactorAux per point
int form_column_code(CacheForm f) {  // cwbl_column_reuse_info_t::form
  return f == CacheForm::Records      ? CWBL_COLUMN_FORM_RECORDS
         : f == CacheForm::WaveFactor ? CWBL_COLUMN_FORM_WAVE
         : f == CacheForm::BigFactor  ? CWBL_COLUMN_FORM_BIG
                                      : CWBL_COLUMN_FORM_NONE;
}
struct CacheKey {
  unsigned long long gen;  // State::gen: obs set, cwbl_init constants, options
  int kp;                  // the path's KP (the record path: kTq4KP)
  float multi_infl;        // inflat is on the record's diagonal
  int dims[7];             // nx, ny, nz, alt_nx, alt_ny, ix_lim, iy_lim (per column: nz, alt 0)
  cwbl_type_params gts[CWBL_NUM_GTS_TYPES], radar[CWBL_NUM_RADAR_TYPES];
};
struct Cache {
  const bool per_column;  // the column cache: a unit is a column of a shared call, not a point
  bool valid = false;     // a fill completed: everything below describes it
  CacheKey key{};
  // Batch b < off.size() of `plan` (the leading batches that fit the budget) keeps its nb
  // records and the spare one that solve_tq40_kernel's lanes past a launch read, from word
  // off[b] of `rec`; sub-batch s0 of it starts s0 records on, its spare being the next
  // sub-batch's first record.  info: (p, level) of the `units` cached points or columns as the
  // fill left them; a hit restores p.  sx, sy, salt: the coordinates the records were assembled
  // from (per column: no alt, nalt = 0).
  // aux (form Tq40Factor only): one FactorAux per record of `rec`, spares included, by the same
  // ordinal: batch b's entries start at entry off[b] / WORDS, sub-batch s0's s0 entries on.
  DevBuf rec, aux, info, sx, sy, salt, flag;
  PinBuf hflag;
  CacheForm form = CacheForm::None;  // what the allocation last served (begin_cache_fill)
  size_t words() const { return form_words(form, key.kp); }  // fp64 words of a record
  std::vector<std::pair<long long, int>> plan;
  std::vector<size_t> off;
  long long units = 0;
  size_t nxy = 0, nalt = 0;
  // what a call that skips plan_trees and the searches still reports (lz_truncated: per level
  // of the filling call, which a per-point call has one of)
  int nt = 0, list_cap = 0;
  long long lz_truncated = 0, q1_undefined = 0;
  size_t bytes() const { return rec.n + aux.n + info.n + sx.n + sy.n + salt.n + flag.n; }
  void release() {
    valid = false;
    form = CacheForm::None;
    for (DevBuf *b : {&rec, &aux, &info, &sx, &sy, &salt, &flag}) b->release();
    hflag.release();
    plan.clear();
    off.clear();
    units = 0;
  }
};

struct State {
  bool inited = false;
  int k = 0, kp = 0, device = 0, wf = 0, q1_mode = 0;
  int kp_natural = 0;  // smallest compiled KP >= k (kp: the one the options select)
  float norain = -5.0f;
  size_t ws_bytes = size_t(2) << 30;
  hipStream_t stream = nullptr;
  std::vector<ObsType> obs;  // gts entries first (family 0), then radar (family 1)
  bool have_obs = false;
  std::vector<std::unique_ptr<TreeBufs>> tree_cache;  // trees of the current obs set
  DevBuf tdesc, nbr_cnt, nbr_idx, info, stats;
  DevBuf nbr_cnt2, nbr_idx2;                          // second list buffer (search overlap)
  hipStream_t sstream = nullptr;                      // neighbour searches of later batches
  std::vector<hipEvent_t> cevents;                    // ordering events of the host copies
  int lead_div = 0;                                   // first batch = npts / lead_div (0: off)
  bool serial_search = false;                         // CWBL_DEBUG_SERIAL=1: searches on S.stream
  // Points per search/solve batch.  Measured on C2 (one GPU, ms per variable): 40 k 113,
  // 70 k 110, 100 k 108, 150 k 107, 200 k 106, 500 k 109; and on an eighth of the grid (a
  // rank of the 8-GPU run): 14.7-15.0 up to 150 k, 15.3 at 200 k, 16.6 at 285 k.  Smaller
  // batches keep each batch's lists and hand-off records nearer the caches and overlap
  // more of the search; below ~70 k the per-batch fixed costs win.
  long long max_batch = 160000;
  bool max_batch_set = false;
  // one-stream path: the per-point info (solved, p) of a window of up to info_window points
  // is reduced once per window (a reduction kernel per batch cost the C2 step ~0.5 ms)
  long long info_window = 1LL << 25;  // 256 MB of int2 (CWBL_OPT_INFO_WINDOW)                         // CWBL_OPT_MAX_BATCH given: no ~6-batch rule
  DevBuf sx, sy, salt, svar;                          // slab staging (host-memory calls)
  DevBuf bcol, byo, byb, bxb, bxa, bev, btri;         // solve_batch staging (btri: T per point)
  DevBuf qxyz, qnf, qidx, qr2;                        // search staging
  DevBuf quad;                                        // x^-1/2 quadrature tables
  DevBuf wsa;                                         // hand-off records (split KP=40 path)
  DevBuf wsf;  // CWBL_OPT_COLUMN_FACTOR: the factors of a (sub-)batch's columns, for the call
  DevBuf flags;                                       // binned search: flagged points (+ count)
  int index_mode = 0;                                 // CWBL_OPT_INDEX
  int index_order = 0;                                // CWBL_OPT_INDEX_ORDER
  DevBuf tdesc_tree;                                  // index mode 1: the tree searches' table
  DevBuf ix_keys[2], ix_vals[2], ix_hist, ix_part;    // device bin build scratch
  PinBuf ix_pin;                                      // its bounds read-back; the flag counts
  std::vector<hipEvent_t> pevents;                    // cwbl_prep_info timing
  bool binned = true;                                 // CWBL_OPT_SEARCH = 1: k-d tree search only
  int bin_div = 0;  // CWBL_OPT_BIN_DIV: bin side = radius / bin_div (0: by density, bin_div_for)
  bool pageable_register = true;                      // CWBL_OPT_PAGEABLE = 1: bounce slots
  bool jacobi = false;                                // CWBL_OPT_SOLVER = 1: Jacobi eigen path
  int tq4 = 1;  // CWBL_OPT_SPLIT40: KP=40 solve 0 = one kernel, else assembly record + solve_tq40
  long long tq4_sub = 0;                              // CWBL_TQ4_SUB: record batch (points)
  bool big_split = true;                              // big_path 1: hand-off + one-wave tail
  long long big_sub = 98304;                          // CWBL_OPT_BIG_BATCH: k > 64 sub-batch
  std::vector<hipEvent_t> events;
  hipStream_t h2d = nullptr, d2h = nullptr;           // host-memory slab copies (pipelined)
  hipStream_t caller_stream = nullptr;                // cwbl_set_stream (null: legacy stream)
  hipEvent_t order_ev = nullptr;                      // order_after_caller
  // cwbl_set_kernel_timing: every solve/search launch of cwbl_analyze_var bracketed by a HIP
  // event pair on the stream it runs on; summed per kernel after the call's final sync
  bool ktiming = false;
  KTime ktime[KT_COUNT];
  std::vector<hipEvent_t> kevents;
  int kev_used = 0;
  struct KPend { int id; hipEvent_t e0, e1; long long pts; };
  std::vector<KPend> kpend;
  size_t handoff_budget = 0;                          // bytes for the k > 64 hand-off records
  unsigned long long gen = 0;     // bumped by cwbl_init, cwbl_set_obs and cwbl_set_option
  size_t reuse_budget = 0;        // CWBL_OPT_RECORD_REUSE in bytes (0: no reuse)
  bool factor_reuse = true;       // CWBL_OPT_FACTOR_REUSE: the cache keeps factors, not records
  bool hit_merge = true;          // CWBL_OPT_HIT_MERGE: one hit launch per info window
  bool wave_reuse = false;        // CWBL_OPT_WAVE_REUSE: the factor cache of k = 41..64
  bool big_reuse = false;         // CWBL_OPT_BIG_REUSE: the factor cache of k = 65..96
  bool rows_reuse = false;        // CWBL_OPT_ROWS_REUSE: the factor cache of k = 97..128
  bool host_pipe = false;         // CWBL_OPT_HOST_PIPE: group, column-shared and tune_q calls
                                  // pipe their host slabs per batch
  // the segment tables of a call's merged hit launches (HitSeg): written by the host, one
  // asynchronous copy per launch
  DevBuf hitseg;
  PinBuf hitseg_pin;
  int column_share = 0;           // CWBL_OPT_COLUMN_SHARE: 0 off, 1 column kernel, 2 chunks only
  int column_levels = 0;          // CWBL_OPT_COLUMN_LEVELS: levels per wave (0: automatic)
  bool column_factor = false;     // CWBL_OPT_COLUMN_FACTOR: a shared call's levels from one kept
                                  // factor per column (k = 41..96)
  bool column_rows = false;       // CWBL_OPT_COLUMN_ROWS: k = 97..128 is eligible for
                                  // CWBL_OPT_COLUMN_FACTOR and CWBL_OPT_COLUMN_REUSE
  int ncu = 0;                    // compute units of the device (automatic level split)
  size_t column_reuse = 0;        // CWBL_OPT_COLUMN_REUSE in bytes (0: off)
  Cache cache{false};   // the record cache (CWBL_OPT_RECORD_REUSE)
  Cache ccache{true};   // the column cache (CWBL_OPT_COLUMN_REUSE)
  // pageable host slabs: each batch's var columns go through page-locked bounce slots (two
  // in, two out), filled and drained by a few host threads while the GPU runs other batches
  static constexpr int kSlots = 3;
  PinBuf pin_in[kSlots], pin_out[kSlots];
  HostPool pool;
};

State S;

float search_r2() {
  const float gc1999 = 2.0f * std::sqrt(10.0f / 3.0f);  // module_param.f90:116
  return gc1999 * gc1999;                               // module_localization.f90:202
}

bool is_gts_assimilated(int id) {  // module_localization.f90:59-72
  return id == CWBL_GTS_SYNOP || id == CWBL_GTS_METAR || id == CWBL_GTS_SHIPS ||
         id == CWBL_GTS_SOUND || id == CWBL_GTS_GPSPW;
}

int tree_depth(const HostTree &t, int node = 0) {
  if (t.nodes.empty()) return 0;
  int depth = 0;
  // iterative DFS over (node, level)
  std::vector<std::pair<int, int>> st{{node, 1}};
  while (!st.empty()) {
    auto [nd, lv] = st.back();
    st.pop_back();
    depth = std::max(depth, lv);
    if (t.nodes[nd].cut_dim >= 0) {
      st.push_back({t.nodes[nd].left, lv + 1});
      st.push_back({t.nodes[nd].right, lv + 1});
    }
  }
  return depth;
}

// copy an array given by the caller (host or device) into a library device buffer
hipError_t stage(DevBuf &dst, const void *src, size_t bytes, int memory) {
  hipError_t e = dst.ensure(bytes);
  if (e != hipSuccess || bytes == 0) return e;
  return hipMemcpyAsync(dst.p, src, bytes,
                        memory == CWBL_MEM_DEVICE ? hipMemcpyDeviceToDevice
                                                  : hipMemcpyHostToDevice,
                        S.stream);
}

hipError_t cevent(int i, hipEvent_t *out) {  // ordering events (timing off)
  while ((int)S.cevents.size() <= i) {
    hipEvent_t e;
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    S.cevents.push_back(e);
  }
  *out = S.cevents[i];
  return hipSuccess;
}

hipError_t event(int i, hipEvent_t *out) {
  while ((int)S.events.size() <= i) {
    hipEvent_t e;
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return r;
    S.events.push_back(e);
  }
  *out = S.events[i];
  return hipSuccess;
}

float elapsed(int a, int b) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, S.events[a], S.events[b]) != hipSuccess) return 0.0f;
  return ms;
}

// Kernel timing (cwbl_set_kernel_timing): kt_begin records the first event of a launch's
// pair on its stream (-1 when timing is off), kt_end the second, queued for kt_collect.
hipError_t kt_event(int i, hipEvent_t *out) {
  while ((int)S.kevents.size() <= i) {
    hipEvent_t e;
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return r;
    S.kevents.push_back(e);
  }
  *out = S.kevents[i];
  return hipSuccess;
}

hipError_t kt_begin(hipStream_t s, int *ev) {
  *ev = -1;
  if (!S.ktiming) return hipSuccess;
  hipEvent_t e;
  hipError_t r = kt_event(S.kev_used, &e);
  if (r != hipSuccess) return r;
  *ev = S.kev_used;
  S.kev_used += 2;
  return hipEventRecord(e, s);
}

hipError_t kt_end(hipStream_t s, int ev, int id, long long pts) {
  if (ev < 0) return hipSuccess;
  hipEvent_t e;
  hipError_t r = kt_event(ev + 1, &e);
  if (r != hipSuccess) return r;
  S.kpend.push_back({id, S.kevents[ev], e, pts});
  return hipEventRecord(e, s);
}

// Two launches back to back on one stream between events the call records anyway (e0 before
// the first, e1 after the second): one more event between them times both.  Each event
// between two kernels costs the stream ~5 us (r4: 4 per C2 batch were 0.9% of the step).
hipError_t kt_pair(hipStream_t s, hipEvent_t e0, int id0, long long pts0, hipEvent_t e1,
                   int id1, long long pts1, const std::function<hipError_t()> &first,
                   const std::function<hipError_t()> &second) {
  hipError_t r = first();
  if (r != hipSuccess) return r;
  if (S.ktiming) {
    hipEvent_t mid;
    r = kt_event(S.kev_used++, &mid);
    if (r != hipSuccess) return r;
    r = hipEventRecord(mid, s);
    if (r != hipSuccess) return r;
    S.kpend.push_back({id0, e0, mid, pts0});
    S.kpend.push_back({id1, mid, e1, pts1});
  }
  return second();
}

void kt_collect() {  // after the call's final synchronisation
  for (const State::KPend &p : S.kpend) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, p.e0, p.e1) != hipSuccess) continue;
    KTime &t = S.ktime[p.id];
    t.launches += 1;
    t.points += p.pts;
    t.ms += ms;
  }
  S.kpend.clear();
  S.kev_used = 0;
}

std::string kernel_name(int id) {
  const std::string kp = std::to_string(S.kp);
  switch (id) {
    case KT_SEARCH_BINNED: return "search_binned_kernel";
    case KT_SEARCH_FLAGGED: return "search_kernel<FlagQuery>";
    case KT_SEARCH_TREE: return "search_kernel<SlabQuery>";
    case KT_ASSEMBLE_RECORD: return "assemble_record_kernel<" + std::to_string(kRecordWaves) + ">";
    case KT_SOLVE_TQ40: return "solve_tq40_kernel<" + kp + ", 0>";
    case KT_SOLVE_TQ40_MULTI: return "solve_tq40_multi_kernel<" + kp + ">";
    case KT_SOLVE_TQ40_COLUMN: return "solve_tq40_column_kernel<" + kp + ">";
    case KT_FILL_TQ40_FACTOR: return "fill_tq40_factor_kernel<" + kp + ">";
    case KT_SOLVE_TQ40_FACTOR: return "solve_tq40_factor_kernel<" + kp + ">";
    case KT_FILL_TQ_WAVE: return "fill_tq_wave_kernel<" + kp + ">";
    case KT_SOLVE_TQ_WAVE_FACTOR: return "solve_tq_wave_factor_kernel<" + kp + ">";
    case KT_BIG_HANDOFF:
      return S.kp == 128 ? "solve_tq_rows_kernel<128, 64>"
                         : "solve_tq_big_kernel<" + kp + ", false, " +
                               std::to_string(big_split_j0(S.kp)) + ">";
    case KT_TQB_TAIL:
      return "solve_tqb_tail_kernel<" + kp + ", " + std::to_string(big_split_j0(S.kp)) +
             (S.kp == 128 ? ", 3>" : ", 2>");
    case KT_FILL_TQB_TAIL:
      return "fill_tqb_tail_kernel<" + kp + ", " + std::to_string(big_split_j0(S.kp)) + ">";
    case KT_SOLVE_TQB_FACTOR:
      return "solve_tqb_factor_kernel<" + kp + ", " + std::to_string(big_split_j0(S.kp)) + ">";
    case KT_BIG_HANDOFF_MULTI2:
    case KT_BIG_HANDOFF_MULTI4:
    case KT_BIG_HANDOFF_MULTI8: {
      const std::string nv = std::to_string(2 << (id - KT_BIG_HANDOFF_MULTI2));
      return (S.kp == 128 ? "solve_tq_rows_multi_kernel<128, 64, "
                          : "solve_tq_big_multi_kernel<96, 32, ") + nv + ">";
    }
    case KT_TQB_TAIL_MULTI2:
    case KT_TQB_TAIL_MULTI4:
    case KT_TQB_TAIL_MULTI8:
      return "solve_tqb_tail_multi_kernel<" + kp + ", " + std::to_string(big_split_j0(S.kp)) +
             ", " + std::to_string(2 << (id - KT_TQB_TAIL_MULTI2)) + ">";
    case KT_SOLVE_TQ: return "solve_tq_kernel<" + kp + ", false>";
    case KT_SOLVE_TQ_MULTI2: return "solve_tq_multi_kernel<" + kp + ", 2>";
    case KT_SOLVE_TQ_MULTI4: return "solve_tq_multi_kernel<" + kp + ", 4>";
    case KT_SOLVE_TQ_MULTI8: return "solve_tq_multi_kernel<" + kp + ", 8>";
    case KT_SOLVE_TQ_BIG: return "solve_tq_big_kernel<" + kp + ", false>";
    case KT_SOLVE_JACOBI: return "solve_kernel<" + kp + ", false>";
    case KT_TUNE_Q: return "tune_q_kernel";
    case KT_SOLVE_TQ_WAVE_FACTOR_COLUMN: return "solve_tq_wave_factor_column_kernel<" + kp + ">";
    case KT_SOLVE_TQB_FACTOR_COLUMN:
      return "solve_tqb_factor_column_kernel<" + kp + ", " + std::to_string(big_split_j0(S.kp)) +
             ">";
    case KT_SOLVE_TQ_WAVE_FACTOR_COLUMN_ALL:
      return "solve_tq_wave_factor_column_all_kernel<" + kp + ">";
    case KT_SOLVE_TQB_FACTOR_COLUMN_ALL:
      return "solve_tqb_factor_column_all_kernel<" + kp + ", " +
             std::to_string(big_split_j0(S.kp)) + ">";
  }
  return "?";
}

// page-locked (hipHostMalloc'd or hipHostRegister'ed) host memory: DMA-able as it is
bool host_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// k rows of nb floats between a member-slowest host slab (row pitch L) and a packed slot
double g_bounce_ms = 0.0;  // host time in the bounce copies of the current call
void bounce_rows(HostPool &pool, float *slot, float *var, long long L, long long g0, int nb,
                 int k, bool to_slot) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t row = (size_t)nb * 4;
  pool.run(k, [&](int m) {
    float *h = var + (size_t)m * L + g0, *b = slot + (size_t)m * nb;
    if (to_slot) std::memcpy(b, h, row);
    else std::memcpy(h, b, row);
  });
  g_bounce_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int require_device() {
  if (!S.inited) return fail(CWBL_ERR_STATE, "cwbl_init has not been called");
  return CWBL_OK;
}

// The library's streams are non-blocking: they are not ordered after work the caller has
// queued on its own stream.  Every entry point that reads or writes caller device memory
// therefore first makes the library's stream wait for an event recorded on the caller's
// stream (cwbl_set_stream; the legacy null stream by default), so device buffers may be
// passed as soon as their producers have been *queued* there.  Only that stream is waited
// for: unrelated streams of the process (another rank's collectives, other compute) are not
// (host-memory calls need no wait: the caller's host arrays are complete when the call is
// made).
hipError_t order_after_caller() {
  if (!S.order_ev) {
    hipError_t e = hipEventCreateWithFlags(&S.order_ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipEventRecord(S.order_ev, S.caller_stream);
  if (e != hipSuccess) return e;
  return hipStreamWaitEvent(S.stream, S.order_ev, 0);
}

// Bin side r / div for the uniform-bin search: r/2 by default; r/4 where the obs are dense
// (more than 24 per r/2 cell on average over the set's bounding box: the finer cells trim
// the per-row runs closer to the ball).  r4 A/B: C5 (49 per r/2 cell) 15.95 M pts/s at r/2,
// 16.04 at r/3, 16.19 at r/4; C2 (~11 per cell) 59.4 / 58.9 / 58.6.  CWBL_OPT_BIN_DIV forces it.
int bin_div_density(int n, const float lo[3], const float hi[3], int dim) {
  if (n == 0) return 2;
  const double h = 0.5 * std::sqrt((double)search_r2());
  double cells = 1.0;
  for (int c = 0; c < dim; ++c) cells *= std::max(1.0, ((double)hi[c] - (double)lo[c]) / h);
  return (double)n / cells > 24.0 ? 4 : 2;
}

int bin_div_for(const HostTree &t, int dim) {
  if (S.bin_div > 0) return S.bin_div;
  const int n = t.n;
  if (n == 0) return 2;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool seen = false;
  for (int i = 0; i < n; ++i) {
    const float *d = &t.rdata[4 * (size_t)i];
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || (dim == 3 && !std::isfinite(d[2]))) continue;
    for (int c = 0; c < dim; ++c) {
      lo[c] = seen ? std::min(lo[c], d[c]) : d[c];
      hi[c] = seen ? std::max(hi[c], d[c]) : d[c];
    }
    seen = true;
  }
  return bin_div_density(n, lo, hi, dim);
}

cwbl_reuse_info_t R;  // cwbl_reuse_info: what the current cwbl_analyze_var reused
cwbl_column_info_t CI;  // cwbl_column_info: what it shared per column (CWBL_OPT_COLUMN_SHARE)
cwbl_column_reuse_info_t CR;  // cwbl_column_reuse_info: what it did with the column cache
cwbl_transfer_info_t TI;  // cwbl_transfer_info: how it moved a host slab's var

// ---- cwbl_prep_info: what the current cwbl_analyze_var spends on its search index -----------
cwbl_prep_info_t P;
// ---- cwbl_index_info / cwbl_index_slots: how the current cwbl_analyze_var numbers its columns --
cwbl_index_info_t IX;
struct IndexUse { int family, type_id; TreeBufs *tb; };  // tb lives until release_obs
std::vector<IndexUse> g_index_use;
bool g_index_called = false;
struct PrepSpan { int ev; int kind; };  // kind 0: bins (device build), 1: columns
std::vector<PrepSpan> g_pspans;
int g_pev_used = 0;

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

hipError_t prep_begin(hipStream_t s, int kind) {
  while ((int)S.pevents.size() < g_pev_used + 2) {
    hipEvent_t e;
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return r;
    S.pevents.push_back(e);
  }
  g_pspans.push_back({g_pev_used, kind});
  g_pev_used += 2;
  return hipEventRecord(S.pevents[g_pspans.back().ev], s);
}

hipError_t prep_end(hipStream_t s) { return hipEventRecord(S.pevents[g_pspans.back().ev + 1], s); }

void prep_collect() {  // after a synchronisation of S.stream
  for (const PrepSpan &p : g_pspans) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, S.pevents[p.ev], S.pevents[p.ev + 1]) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    (p.kind == 0 ? P.ms_bins : P.ms_columns) += ms;
  }
  g_pspans.clear();
  g_pev_used = 0;
}

// The device bin build (cwbl_index.hip) of n > 0 points on stream s.  have_bounds: `bounds` is
// that of an earlier build of the same coordinates (ncoord is then current too); otherwise
// dxyz(3,n) is normalised into ncoord and the bounds are reduced and read back (one
// synchronisation of s).  div_opt: the divisor, 0 = by density.  Fills the grid of `bins`
// and, unless grid_only, bxyz / bstart; *skeys / *svals (nullable) point at the sorted cell
// ids and obs indices in the scratch buffers, valid until the next build.  by_position: the
// payload of bxyz[p] is p, not the obs index (CWBL_OPT_INDEX_ORDER = 1).
int device_bins(hipStream_t s, const float *dxyz, int n, int tdim, float hinv, float vinv,
                int div_opt, bool have_bounds, IndexBounds &bounds, DevBuf &ncoord,
                HostBins &bins, int &div_used, bool grid_only, DevBuf *bxyz, DevBuf &bstart,
                const int **skeys = nullptr, const int **svals = nullptr,
                bool by_position = false) {
  if (!have_bounds) {
    const int nblk = index_bound_blocks(n);
    const size_t pbytes = (size_t)nblk * kIndexBoundWords * sizeof(float);
    HIPCHK(ncoord.ensure((size_t)n * sizeof(float4)));
    HIPCHK(S.ix_part.ensure(pbytes));
    HIPCHK(S.ix_pin.ensure(std::max<size_t>(pbytes, 64)));
    HIPCHK(launch_index_normalize(s, dxyz, n, tdim, hinv, vinv, ncoord.as<float4>(),
                                  S.ix_part.as<float>()));
    HIPCHK(hipMemcpyAsync(S.ix_pin.p, S.ix_part.p, pbytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    index_finish_bounds(S.ix_pin.as<float>(), nblk, bounds);
  }
  div_used = div_opt > 0 ? div_opt : bin_div_density(n, bounds.alo, bounds.ahi, tdim);
  bin_grid(bounds.lo, bounds.hi, tdim, std::sqrt(search_r2()), div_used, bins);
  if (grid_only) return CWBL_OK;
  const int ncell = bins.nbx * bins.nby * bins.nbz;
  for (int i = 0; i < 2; ++i) {
    HIPCHK(S.ix_keys[i].ensure((size_t)n * sizeof(int)));
    HIPCHK(S.ix_vals[i].ensure((size_t)n * sizeof(int)));
  }
  HIPCHK(S.ix_hist.ensure((size_t)index_sort_blocks(n) * 256 * sizeof(int)));
  if (bxyz) HIPCHK(bxyz->ensure(((size_t)n + kBinPad) * sizeof(float4)));
  HIPCHK(bstart.ensure(((size_t)ncell + 1) * sizeof(int)));
  int *keys[2] = {S.ix_keys[0].as<int>(), S.ix_keys[1].as<int>()};
  int *vals[2] = {S.ix_vals[0].as<int>(), S.ix_vals[1].as<int>()};
  const IndexGrid g{bins.x0, bins.y0, bins.z0, bins.binv, bins.nbx, bins.nby, bins.nbz};
  int which = 0;
  HIPCHK(launch_index_sort(s, n, ncell, ncoord.as<float4>(), tdim, g, keys, vals,
                           S.ix_hist.as<int>(), &which));
  HIPCHK(launch_index_finish(s, ncoord.as<float4>(), n, ncell, keys[which], vals[which],
                             bxyz ? bxyz->as<float4>() : nullptr, bstart.as<int>(), by_position));
  if (skeys) *skeys = keys[which];
  if (svals) *svals = vals[which];
  return CWBL_OK;
}

// The host worker of a mode-1 tree: build_tree's normalisation and kdtree2_create, host work
// only (the calling thread makes every HIP call).  ot.xyz stays put until release_obs, which
// joins the worker first.
void start_tree_worker(TreeBufs *tb, const ObsType &ot, bool dim3) {
  const float *xyz = ot.xyz.data();
  const int n = ot.nobs, tdim = dim3 ? 3 : 2;
  const float hinv = tb->hinv, vinv = tb->vinv;
  tb->worker_started = true;
  tb->worker_joined = false;
  ++P.trees_built;
  tb->worker = std::thread([tb, xyz, n, tdim, dim3, hinv, vinv] {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<float> nx(3 * (size_t)n);
    for (int j = 0; j < n; ++j) {
      nx[3 * (size_t)j + 0] = xyz[3 * (size_t)j + 0] * hinv;
      nx[3 * (size_t)j + 1] = xyz[3 * (size_t)j + 1] * hinv;
      nx[3 * (size_t)j + 2] = dim3 ? xyz[3 * (size_t)j + 2] * vinv : -1.0f;
    }
    build_kdtree(nx.data(), n, tdim, tb->host);
    tb->depth = tree_depth(tb->host);
    tb->worker_ms = ms_since(t0);
  });
}

// Cell order: the uploaded tree's ind as sorted positions, ind2 = rank[ind], on stream s (rank
// was written on S.stream before anything was queued on the search stream).
int compose_ind(TreeBufs *tb, hipStream_t s) {
  const size_t n = tb->host.ind.size();
  HIPCHK(tb->ind2.ensure(n * sizeof(int) + 4));
  HIPCHK(launch_index_compose(s, tb->ind.as<int>(), tb->rank.as<int>(), (int)n,
                              tb->ind2.as<int>()));
  ++IX.trees_composed;
  return CWBL_OK;
}

// Joins a mode-1 tree's worker and uploads the tree on stream s (once).
int ready_tree(TreeBufs *tb, hipStream_t s) {
  if (tb->tree_ready) return CWBL_OK;
  if (!tb->worker_joined) {
    const auto t0 = std::chrono::steady_clock::now();
    tb->join();
    P.ms_tree_wait += ms_since(t0);
    P.ms_tree += tb->worker_ms;
  }
  if (tb->depth >= kSearchStackDepth)
    return fail(CWBL_ERR_UNSUPPORTED, "k-d tree too deep (%d obs)", tb->n);
  const HostTree &h = tb->host;
  HIPCHK(tb->nodes.ensure(std::max<size_t>(h.nodes.size(), 1) * sizeof(TreeNode)));
  HIPCHK(tb->rdata.ensure(h.rdata.size() * sizeof(float)));
  HIPCHK(tb->ind.ensure(h.ind.size() * sizeof(int) + 4));
  HIPCHK(hipMemcpyAsync(tb->nodes.p, h.nodes.data(), h.nodes.size() * sizeof(TreeNode),
                        hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(tb->rdata.p, h.rdata.data(), h.rdata.size() * sizeof(float),
                        hipMemcpyHostToDevice, s));
  if (!h.ind.empty())
    HIPCHK(hipMemcpyAsync(tb->ind.p, h.ind.data(), h.ind.size() * sizeof(int),
                          hipMemcpyHostToDevice, s));
  if (tb->cell_order)
    if (int rc = compose_ind(tb, s)) return rc;
  tb->tree_ready = true;
  return CWBL_OK;
}

// CWBL_OPT_INDEX = 1: the cache entry of one normalisation, its bins built on the device
// (rebuilt alone when the divisor changes), its tree left to a worker when the type can
// truncate (or is searched by tree walk).
int index_entry(int entry, int tdim, bool dim3, float hinv, float vinv, int max_lz,
                TreeBufs *&out) {
  ObsType &ot = S.obs[entry];
  const int n = ot.nobs;
  TreeBufs *tb = nullptr;
  for (auto &t : S.tree_cache)
    if (t->mode == 1 && t->entry == entry && t->dim == tdim && t->hinv == hinv &&
        (!dim3 || t->vinv == vinv) && t->cell_order == S.index_order)
      tb = t.get();
  const bool fresh = !tb;
  if (fresh) {
    auto nt = std::make_unique<TreeBufs>();
    nt->mode = 1; nt->entry = entry; nt->dim = tdim; nt->hinv = hinv; nt->vinv = vinv;
    nt->n = n;
    nt->cell_order = S.index_order;
    tb = nt.get();
    S.tree_cache.push_back(std::move(nt));
  }
  // the tree first: the worker builds it while the device builds the bins
  if (!tb->worker_started && (!S.binned || n > max_lz)) start_tree_worker(tb, ot, dim3);
  if (fresh || tb->bin_div_opt != S.bin_div) {
    if (!ot.dxyz_ok) {
      HIPCHK(ot.dxyz.ensure(ot.xyz.size() * sizeof(float)));
      HIPCHK(hipMemcpyAsync(ot.dxyz.p, ot.xyz.data(), ot.xyz.size() * sizeof(float),
                            hipMemcpyHostToDevice, S.stream));
      ot.dxyz_ok = true;
    }
    HIPCHK(prep_begin(S.stream, 0));
    const int *svals = nullptr;
    if (int rc = device_bins(S.stream, ot.dxyz.as<float>(), n, tdim, hinv, vinv, S.bin_div,
                             !fresh, tb->bounds, tb->ncoord, tb->bins, tb->bin_div_used, false,
                             &tb->bxyz, tb->bstart, nullptr, &svals, tb->cell_order != 0))
      return rc;
    if (tb->cell_order) {
      // the sorted obs indices leave the scratch buffers: the slot table and its inverse; a
      // tree that is already up (a changed divisor) gets its ind composed anew
      const size_t bytes = (size_t)n * sizeof(int);
      HIPCHK(tb->order.ensure(bytes));
      HIPCHK(tb->rank.ensure(bytes));
      HIPCHK(hipMemcpyAsync(tb->order.p, svals, bytes, hipMemcpyDeviceToDevice, S.stream));
      HIPCHK(launch_index_rank(S.stream, tb->order.as<int>(), n, tb->rank.as<int>()));
      if (tb->tree_ready)
        if (int rc = compose_ind(tb, S.stream)) return rc;
    }
    HIPCHK(prep_end(S.stream));
    tb->bin_div_opt = S.bin_div;
    ++P.bins_built;
    ++P.bins_on_device;
  }
  out = tb;
  return CWBL_OK;
}

// Builds the trees of one family (build_tree, module_localization.f90:35-167) and their
// column tables.  Appends TreeDesc entries.
int build_family(int family, const cwbl_var_params *vp, std::vector<TreeDesc> &descs,
                 int &list_cap, int &max_depth, std::vector<TreeBufs *> &tbs) {
  struct Pending { int entry; int type_id; const cwbl_type_params *tp; float hinv, vinv; };
  std::vector<Pending> pend;
  const int ntypes = family == 0 ? CWBL_NUM_GTS_TYPES : CWBL_NUM_RADAR_TYPES;
  for (int id = 1; id <= ntypes; ++id) {
    int entry = -1;
    for (size_t e = 0; e < S.obs.size(); ++e)
      if (S.obs[e].family == family && S.obs[e].type_id == id) entry = (int)e;
    if (entry < 0 || S.obs[entry].nobs <= 0) continue;
    if (family == 0 && !is_gts_assimilated(id)) continue;
    const cwbl_type_params *tp = family == 0 ? &vp->gts[id - 1] : &vp->radar[id - 1];
    if (!(tp->use_it && tp->hclr > 0.0f)) continue;
    if (tp->max_lz_pts < 0) return fail(CWBL_ERR_ARG, "max_lz_pts < 0 for type %d", id);
    const float hinv = 1.0f / (tp->hclr * 1e3f);
    const float vinv = tp->vclr > 0.0f ? 1.0f / (tp->vclr * 1e3f) : -1.0f;
    pend.push_back({entry, id, tp, hinv, vinv});
  }
  if (pend.empty()) return CWBL_OK;
  const bool fam3d = pend.back().vinv > 0.0f;  // Q1: the leftover vclr_inv (:151)
  for (const Pending &pd : pend) {
    ObsType &ot = S.obs[pd.entry];
    const bool own3d = pd.vinv > 0.0f;
    bool dim3 = S.q1_mode == CWBL_Q1_PER_TYPE ? own3d : fam3d;
    int q1u = 0;
    if (dim3 && !own3d) { dim3 = false; q1u = 1; }
    const int n = ot.nobs;
    const int tdim = dim3 ? 3 : 2;
    TreeBufs *tb = nullptr;
    if (S.index_mode == 1) {
      if (int rc = index_entry(pd.entry, tdim, dim3, pd.hinv, pd.vinv, pd.tp->max_lz_pts, tb))
        return rc;
    }
    for (auto &t : S.tree_cache)
      if (S.index_mode == 0 && t->mode == 0 && t->entry == pd.entry && t->dim == tdim &&
          t->hinv == pd.hinv && (!dim3 || t->vinv == pd.vinv) && t->bin_div_opt == S.bin_div)
        tb = t.get();
    if (!tb) {  // build_tree (:35-167) for this normalisation
      std::vector<float> nx(3 * (size_t)n);
      for (int j = 0; j < n; ++j) {
        nx[3 * j + 0] = ot.xyz[3 * j + 0] * pd.hinv;
        nx[3 * j + 1] = ot.xyz[3 * j + 1] * pd.hinv;
        nx[3 * j + 2] = dim3 ? ot.xyz[3 * j + 2] * pd.vinv : -1.0f;
      }
      auto nt = std::make_unique<TreeBufs>();
      nt->entry = pd.entry; nt->dim = tdim; nt->hinv = pd.hinv; nt->vinv = pd.vinv;
      nt->bin_div_opt = S.bin_div;
      nt->n = n;
      const auto t_tree = std::chrono::steady_clock::now();
      build_kdtree(nx.data(), n, tdim, nt->host);
      nt->depth = tree_depth(nt->host);
      P.ms_tree += ms_since(t_tree);
      ++P.trees_built;
      if (nt->depth >= kSearchStackDepth)
        return fail(CWBL_ERR_UNSUPPORTED, "k-d tree too deep (%d obs)", n);
      const HostTree &h = nt->host;
      HIPCHK(nt->nodes.ensure(h.nodes.size() * sizeof(TreeNode)));
      HIPCHK(nt->rdata.ensure(h.rdata.size() * sizeof(float)));
      HIPCHK(nt->ind.ensure(h.ind.size() * sizeof(int) + 4));
      HIPCHK(hipMemcpyAsync(nt->nodes.p, h.nodes.data(), h.nodes.size() * sizeof(TreeNode),
                            hipMemcpyHostToDevice, S.stream));
      HIPCHK(hipMemcpyAsync(nt->rdata.p, h.rdata.data(), h.rdata.size() * sizeof(float),
                            hipMemcpyHostToDevice, S.stream));
      if (!h.ind.empty())
        HIPCHK(hipMemcpyAsync(nt->ind.p, h.ind.data(), h.ind.size() * sizeof(int),
                              hipMemcpyHostToDevice, S.stream));
      const auto t_bins = std::chrono::steady_clock::now();
      build_bins(h, tdim, std::sqrt(search_r2()), nt->bins, bin_div_for(h, tdim));
      P.ms_bins += ms_since(t_bins);
      ++P.bins_built;
      const HostBins &hb = nt->bins;
      // (+ kBinPad points: search_binned_kernel reads up to 7 points past a run's end)
      HIPCHK(nt->bxyz.ensure(hb.xyzs.size() * sizeof(float) + 16 * kBinPad));
      HIPCHK(nt->bstart.ensure(hb.start.size() * sizeof(int)));
      if (!hb.xyzs.empty())
        HIPCHK(hipMemcpyAsync(nt->bxyz.p, hb.xyzs.data(), hb.xyzs.size() * sizeof(float),
                              hipMemcpyHostToDevice, S.stream));
      HIPCHK(hipMemcpyAsync(nt->bstart.p, hb.start.data(), hb.start.size() * sizeof(int),
                            hipMemcpyHostToDevice, S.stream));
      tb = nt.get();
      S.tree_cache.push_back(std::move(nt));
    }
    const size_t ncol = (size_t)n * ot.nvar;
    HIPCHK(tb->col_bg.ensure(ncol * S.kp * sizeof(float)));
    HIPCHK(tb->col_omm.ensure(ncol * sizeof(float)));
    HIPCHK(tb->col_err.ensure(ncol * sizeof(float)));
    HIPCHK(tb->col_ok.ensure(ncol));
    // point-independent QC columns (letkf_yoyb :429-437 / :497-510)
    const cwbl_type_params *tp = pd.tp;
    int is_assim[5] = {0, 0, 0, 0, 0};
    if (family == 0) {
      for (int v = 0; v < ot.nvar; ++v) is_assim[v] = tp->hclr > 0.0f ? tp->is_assim[v] : 0;
    } else {
      is_assim[0] = tp->hclr > 0.0f ? 1 : 0;
    }
    // (index mode 1: a slot is the obs index, the columns stay in obs order; in cell order
    // they are gathered through `order`, as mode 0 gathers them through the tree's ind)
    const int *slot_obs = tb->mode == 0    ? tb->ind.as<int>()
                          : tb->cell_order ? tb->order.as<int>()
                                           : nullptr;
    HIPCHK(prep_begin(S.stream, 1));
    HIPCHK(launch_obs_prep(S.stream, S.k, S.kp, family, ot.type_id, ot.nvar, n,
                           ot.obs.as<float>(), ot.error.as<float>(), ot.hdxb.as<float>(),
                           ot.qc.as<int>(), tp->err_muti, tp->err_rej, is_assim, S.norain,
                           slot_obs, tb->col_bg.as<float>(),
                           tb->col_omm.as<float>(), tb->col_err.as<float>(),
                           tb->col_ok.as<uint8_t>()));
    HIPCHK(prep_end(S.stream));
    TreeDesc d{};
    if (tb->mode == 1) {  // the solve's table: coordinates by obs index, no tree
      // (cell order: the bins' own points are the coordinates by slot; the solve reads x, y
      // and z of an rdata entry and never its fourth component, which here holds the slot)
      d.rdata = tb->cell_order ? tb->bxyz.as<float4>() : tb->ncoord.as<float4>();
    } else {
      d.nodes = tb->nodes.as<TreeNode>();
      d.rdata = tb->rdata.as<float4>();
      d.ind = tb->ind.as<int>();
    }
    d.col_bg = tb->col_bg.as<float>();
    d.col_omm = tb->col_omm.as<float>();
    d.col_err = tb->col_err.as<float>();
    d.col_ok = tb->col_ok.as<uint8_t>();
    d.hclr_inv = pd.hinv;
    d.vclr_inv = pd.vinv;
    d.tree_dim = dim3 ? 3 : 2;
    d.query3d = own3d ? 1 : 0;
    d.nvar = ot.nvar;
    d.max_lz = tp->max_lz_pts;
    d.list_off = list_cap;
    d.q1_undef = q1u;
    d.bxyz = tb->bxyz.as<float4>();
    d.bstart = tb->bstart.as<int>();
    d.bx0 = tb->bins.x0; d.by0 = tb->bins.y0; d.bz0 = tb->bins.z0; d.binv = tb->bins.binv;
    d.nbx = tb->bins.nbx; d.nby = tb->bins.nby; d.nbz = tb->bins.nbz;
    list_cap += list_span(tp->max_lz_pts);
    if (tb->mode == 0) max_depth = std::max(max_depth, tb->depth);
    descs.push_back(d);
    tbs.push_back(tb);
    g_index_use.push_back({family, ot.type_id, tb});
  }
  return CWBL_OK;
}

void release_obs() {
  g_index_use.clear();
  for (auto &t : S.tree_cache) t->release();
  S.tree_cache.clear();
  for (auto &o : S.obs) {
    o.obs.release(); o.error.release(); o.hdxb.release(); o.qc.release(); o.dxyz.release();
  }
  S.obs.clear();
  S.have_obs = false;
}

void release_all() {
  release_obs();
  for (hipEvent_t e : S.cevents) (void)hipEventDestroy(e);
  S.cevents.clear();
  for (DevBuf *b : {&S.tdesc, &S.nbr_cnt, &S.nbr_idx, &S.nbr_cnt2, &S.nbr_idx2, &S.info, &S.stats, &S.sx,
                    &S.sy, &S.salt, &S.svar, &S.bcol, &S.byo, &S.byb, &S.bxb, &S.bxa, &S.bev, &S.btri,
                    &S.qxyz, &S.qnf, &S.qidx, &S.qr2, &S.quad, &S.wsa, &S.wsf, &S.flags, &S.tdesc_tree,
                    &S.ix_keys[0], &S.ix_keys[1], &S.ix_vals[0], &S.ix_vals[1], &S.ix_hist,
                    &S.ix_part, &S.hitseg})
    b->release();
  S.ix_pin.release();
  S.hitseg_pin.release();
  S.cache.release();
  S.ccache.release();
  for (hipEvent_t e : S.pevents) (void)hipEventDestroy(e);
  S.pevents.clear();
  g_pspans.clear();
  g_pev_used = 0;
  for (hipEvent_t e : S.events) (void)hipEventDestroy(e);
  S.events.clear();
  for (hipEvent_t e : S.kevents) (void)hipEventDestroy(e);
  S.kevents.clear();
  for (int i = 0; i < State::kSlots; ++i) {
    S.pin_in[i].release();
    S.pin_out[i].release();
  }
  S.pool.stop();
  S.kpend.clear();
  S.kev_used = 0;
  S.ktiming = false;
  for (KTime &t : S.ktime) t = KTime{};
  if (S.order_ev) (void)hipEventDestroy(S.order_ev);
  S.order_ev = nullptr;
  S.caller_stream = nullptr;
  if (S.stream) (void)hipStreamDestroy(S.stream);
  S.stream = nullptr;
  if (S.sstream) (void)hipStreamDestroy(S.sstream);
  S.sstream = nullptr;
  for (hipStream_t *st : {&S.h2d, &S.d2h}) {
    if (*st) (void)hipStreamDestroy(*st);
    *st = nullptr;
  }
  S.inited = false;
}

// k = 17..32: the KP = 40 record path (assembly + four-point solve; the padding rows are
// the identity and the steps past k - 2 exact no-ops) beats the one-wavefront KP = 24 / 32
// solves (C2 grid, r2: 91.6 against 134 ms per variable at k = 32; r3: ~75 against 79 / 88
// at k = 20 / 24); at k <= 16 the one-wavefront solve is faster (68 ms)
void select_kp() {
  S.kp = S.kp_natural;
  if ((S.kp == 24 || S.kp == 32) && S.tq4 && !S.jacobi) S.kp = kTq4KP;
}

SolveConsts solve_consts(float inflat, int use_rtpp, float rtpp_a, int use_rtps, float rtps_a) {
  SolveConsts c{};
  c.k = S.k;
  c.kp = S.kp;
  c.weight_function = S.wf;
  c.inflat = inflat;
  c.use_rtpp = use_rtpp;
  c.use_rtps = use_rtps;
  c.rtpp_alpha = rtpp_a;
  c.rtps_alpha = rtps_a;
  c.nmember_inv = 1.0f / (float)S.k;
  c.r2 = search_r2();
  c.max_sweeps = 30;
  c.quad_r = S.quad.as<double2>();
  c.quad = c.quad_r;
#ifdef CWBL_DEBUG_KNOBS  // timing ablations (make DEBUG_KNOBS=1); not in the release library
  if (const char *e = std::getenv("CWBL_DEBUG_MAX_SWEEPS")) c.max_sweeps = std::atoi(e);
  if (const char *e = std::getenv("CWBL_DEBUG_TQ_STOP")) c.debug_stop = std::atoi(e);
  if (const char *e = std::getenv("CWBL_DEBUG_TQ_STEPS")) c.debug_steps = std::atoi(e);
#endif
  return c;
}

// ---- cwbl_analyze_var / cwbl_analyze_vars by stage -------------------------------------------
// One call (analyze_call; letkf_driver's per-variable body, module_letkf_core.f90:59-297):
//   plan_trees      build_tree x2 (cached per obs set) + the QC column tables   (:63-64)
//   stage_slab      the slab in device memory (host slabs staged / piped)
//   plan_batches    search/solve batches
//   per batch       search_batch (S.sstream) -> solve_batch_path (S.stream), with the host
//                   slab's var piped in and out around it (S.h2d / S.d2h)        (:209-240)
//   finish_call     info reduction, tune_q (:253-278), write-back, statistics
// cwbl_analyze_var is a call of one variable; cwbl_analyze_vars on the record path and on the
// one-wavefront path is a group call: nvar variables that share everything but var and the
// epilogue's flags, so the trees, the batches, the searches and the assembly are variable 0's
// and only the solve (solve_tq40_multi_kernel, solve_tq_multi_kernel), tune_q and the host
// slab's var see every variable.  A column-shared call (CWBL_OPT_COLUMN_SHARE: one variable
// whose trees are all 2-D) runs the same stages over the column view of its slab, and its
// solves (solve_batch_column) cover every level of a batch's columns.
struct VarCall {
  const cwbl_var_params *vp = nullptr;  // [nvar]
  const cwbl_slab *sl = nullptr;        // [nvar]
  int nvar = 1;
  bool group = false;
  // var of every variable in device memory (a single call: var[0] = sd.var) and, for a group,
  // the solve's table of per-variable flags
  Tq40Vars tv{};
  long long npts = 0, L = 0;
  SlabDev sd{};
  size_t bvar = 0;
  // host-memory slab: x, y, alt staged first; var piped batch by batch (piped: the analysed
  // region is the whole horizontal slab, so a batch's points are contiguous in every member
  // plane) or moved whole; a pageable var page-locked in place (registered) or, failing that,
  // through the library's page-locked bounce slots.  A group's and a column-shared call's var
  // move whole unless CWBL_OPT_HOST_PIPE pipes them (never through the slots).  reg: the
  // arrays page-locked for the call; tune_batch: tune_q runs per batch, behind its solve, so
  // that a call with tune_q pipes its analysis back as well (CWBL_OPT_HOST_PIPE)
  bool host = false, piped = false, piped_back = false, bounce = false, registered = false;
  bool tune_batch = false;
  std::vector<float *> reg;
  std::vector<TreeDesc> descs;
  // index mode 1: the cache entry of every descriptor, and whether the tree searches' table
  // (S.tdesc_tree: the trees that exist, with their own rdata) has been uploaded
  std::vector<TreeBufs *> tbs;
  bool index1 = false, trees_ready = false;
  int list_cap = 0, max_depth = 1, nt = 0;
  std::vector<std::pair<long long, int>> plan;  // (g0, nb)
  long long B = 0, Bc = 0, info_cap = 0, win0 = 0;
  SolveConsts c{};
  float rbox = 0.0f;
  // timing events S.events[ev..] (four per batch: search begin/end, solve begin/end; under
  // tune_batch a fifth, the end of the batch's tune_q) and
  // ordering events S.cevents[cev..] of the piped copies
  int ev = 4, cev = 0;
  std::vector<std::pair<int, int>> search_ev, solve_ev;
  std::vector<int> done_ev, h2d_done, d2h_done;
  // record reuse: 1 = this call fills the cache, 2 = it solves from it (the leading ncached
  // batches; full_hit: every batch, so no tree, column table or search is needed at all)
  int reuse = 0;
  long long ncached = 0;
  bool full_hit = false;
  // the cache that reuse, ncached and full_hit speak of (null: the call has none); colcache:
  // it is the column cache (CWBL_OPT_COLUMN_REUSE: a column-shared call), not the record cache
  Cache *cache = nullptr;
  bool colcache = false;
  // CWBL_OPT_HIT_MERGE: the call's cached batches go out in one launch per info window;
  // hitseg_used: entries of S.hitseg_pin taken by the launches so far; cuts: the traces at which
  // the call's inflat and k raise a wave's rounds (hit_level_cuts)
  bool merge = false;
  size_t hitseg_used = 0;
  HitLevelCuts cuts = {};
  // CWBL_OPT_COLUMN_SHARE (1 or 2 when the call is shared, else 0): sd is the column view of
  // the slab (nz = 1; L stays the member stride nx ny nz) and npts its ncol = ix_lim iy_lim
  // points, so the plan, the searches, the lists, the assembly and the info windows are per
  // column; `full` is the slab itself, nlev its nz.  lev: levels a solve launch of
  // solve_batch_path covers (its kernel-timing points are points x lev).
  int colshare = 0, nlev = 1, lev = 1;
  long long ncol = 0;
  SlabDev full{};
};

bool record_path() { return S.tq4 && S.kp == kTq4KP && !S.jacobi; }
// one wavefront per point with the default solver: solve_tq_kernel, solve_tq_multi_kernel
bool wave_path() { return !record_path() && S.kp <= kMaxWaveKP && !S.jacobi; }
// the hand-off path (k = 65..128 under CWBL_OPT_BIG_PATH = 1: a 256-thread kernel for the
// assembly and the first steps, a record, the one-wavefront tail kernel) is what a call runs
// (CWBL_OPT_SOLVER does not reach k > 64)
bool handoff_path() {
  return (S.kp == 96 || S.kp == kBigSplitKP) && S.big_split && S.k > big_split_j0(S.kp) + 2;
}
// the one-wavefront path's calls that fill and read the factor cache (CWBL_OPT_WAVE_REUSE;
// accepted and ignored at the smaller KP)
bool wave_reuse_path() { return S.wave_reuse && wave_path() && S.kp > kTq4KP; }
// the hand-off path's calls that fill and read the factor cache (CWBL_OPT_BIG_REUSE at KP = 96,
// CWBL_OPT_ROWS_REUSE at KP = 128; each accepted and ignored at the other KP and on every other
// path)
bool big_reuse_path() {
  return handoff_path() && (S.kp == 96 ? S.big_reuse : S.kp == kBigSplitKP && S.rows_reuse);
}
// the form that a single-variable call on the current path and options fills and reads
CacheForm call_form() {
  if (record_path()) return S.factor_reuse ? CacheForm::Tq40Factor : CacheForm::Records;
  if (wave_reuse_path()) return CacheForm::WaveFactor;
  if (big_reuse_path()) return CacheForm::BigFactor;
  return CacheForm::None;
}

void make_cache_key(CacheKey &key, const cwbl_var_params *vp, const cwbl_slab *sl,
                    bool per_column) {
  std::memset(&key, 0, sizeof key);
  key.gen = S.gen;
  key.kp = S.kp;
  key.multi_infl = vp->multi_infl;
  const int dims[7] = {sl->nx, sl->ny, per_column ? 0 : sl->nz, per_column ? 0 : sl->alt_nx,
                       per_column ? 0 : sl->alt_ny, sl->ix_lim, sl->iy_lim};
  std::memcpy(key.dims, dims, sizeof dims);
  std::memcpy(key.gts, vp->gts, sizeof key.gts);
  std::memcpy(key.radar, vp->radar, sizeof key.radar);
}

size_t cache_budget(const Cache &C) { return C.per_column ? S.column_reuse : S.reuse_budget; }

// The hit test behind an equal key: the slab's coordinates (staged copies for a host slab)
// against the fill's snapshot, exactly.  A caller may have rewritten x, y or alt in place
// behind unchanged pointers.  (The column cache snapshots no alt, nalt = 0: nothing is
// launched for it.)  One flag read back, one synchronisation of S.stream.
int cache_coords_match(VarCall &v, Cache &C, bool &same) {
  const auto t0 = std::chrono::steady_clock::now();
  int *flag = C.flag.as<int>();
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), S.stream));
  HIPCHK(launch_coord_snapshot(S.stream, false, v.sd.x, C.sx.as<float>(), (long long)C.nxy, flag));
  HIPCHK(launch_coord_snapshot(S.stream, false, v.sd.y, C.sy.as<float>(), (long long)C.nxy, flag));
  HIPCHK(launch_coord_snapshot(S.stream, false, v.sd.alt, C.salt.as<float>(), (long long)C.nalt,
                               flag));
  HIPCHK(hipMemcpyAsync(C.hflag.p, flag, sizeof(int), hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  same = *C.hflag.as<int>() == 0;
  (C.per_column ? CR.ms_compare : R.ms_compare) = ms_since(t0);
  return CWBL_OK;
}

// A call of the cache v.cache whose key or coordinates differ from the cache's: plans which
// leading batches' records fit the budget, allocates what they need (kept from an earlier fill
// when it is large enough) and takes the coordinate snapshot.  The batches then assemble, or
// fill their factors, into their own regions instead of S.wsa or S.wsf.  A failed allocation is
// no error: nothing is held and the call runs without reuse.
int begin_cache_fill(VarCall &v, const CacheKey &key, CacheForm form) {
  Cache &C = *v.cache;
  const size_t budget = cache_budget(C);
  C.valid = false;
  C.key = key;
  C.plan = v.plan;
  C.off.clear();
  C.units = 0;
  C.form = form;
  size_t words = 0;
  for (const auto &b : v.plan) {
    // (+1: the spare record; the wave kernels read none, the region's layout is one)
    const size_t need = ((size_t)b.second + 1) * C.words();
    if ((words + need) * sizeof(double) > budget) break;
    C.off.push_back(words);
    words += need;
    C.units += b.second;
  }
  if (C.off.empty()) {
    // no batch fits: the record cache keeps an earlier fill's buffers for the next one, the
    // column cache holds nothing
    if (C.per_column) C.release();
    return CWBL_OK;
  }
  const cwbl_slab *sl = v.sl;
  C.nxy = (size_t)sl->nx * sl->ny;
  C.nalt = C.per_column ? 0 : (size_t)sl->alt_nx * sl->alt_ny * sl->nz;
  // Grow-only, with 1/16 of headroom within the budget: the slabs of one cycle differ by a
  // staggered row, column or level (2 % at 300 x 300 x 50), and replacing the buffer is dear
  // (bench.py's cycle leg once lost 1.6 s to the regrow of 31 GB for a 51-level slab)
  const size_t need = words * sizeof(double);
  bool ok = need <= C.rec.n || C.rec.ensure(std::min(budget, need + need / 16)) == hipSuccess;
  // The steps' scalars of the factors, an entry per record: beside the budget's cut, like info
  // and the snapshot, with the same headroom; a cache of records holds none
  if (form_has_aux(form)) {
    const size_t aneed =
        words / AsmRecord<kTq4KP>::WORDS * FactorAux<kTq4KP>::WORDS * sizeof(double);
    ok = ok && (aneed <= C.aux.n || C.aux.ensure(aneed + aneed / 16) == hipSuccess);
  } else {
    C.aux.release();
  }
  ok = ok && C.info.ensure((size_t)C.units * sizeof(int2)) == hipSuccess;
  ok = ok && C.sx.ensure(C.nxy * 4) == hipSuccess && C.sy.ensure(C.nxy * 4) == hipSuccess;
  ok = ok && C.salt.ensure(C.nalt * 4) == hipSuccess && C.flag.ensure(sizeof(int)) == hipSuccess;
  ok = ok && C.hflag.ensure(64) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    C.release();
    return CWBL_OK;
  }
  HIPCHK(launch_coord_snapshot(S.stream, true, v.sd.x, C.sx.as<float>(), (long long)C.nxy, nullptr));
  HIPCHK(launch_coord_snapshot(S.stream, true, v.sd.y, C.sy.as<float>(), (long long)C.nxy, nullptr));
  HIPCHK(launch_coord_snapshot(S.stream, true, v.sd.alt, C.salt.as<float>(), (long long)C.nalt,
                               nullptr));
  v.reuse = 1;
  v.ncached = (long long)C.off.size();
  return CWBL_OK;
}

// The info window that opens at point g on a hit: the cached points' accepted counts, which
// solve_tq40_kernel reads where the assembly would have left them.
int restore_info(VarCall &v, long long g) {
  if (v.reuse != 2) return CWBL_OK;
  const int2 *const kept = v.cache->info.as<int2>();
  const long long n = std::min<long long>(v.info_cap, v.cache->units - g);
  if (n <= 0) return CWBL_OK;
  HIPCHK(hipMemcpyAsync(S.info.p, kept + g, (size_t)n * sizeof(int2),
                        hipMemcpyDeviceToDevice, S.stream));
  return CWBL_OK;
}

// The info window [v.win0, end) as a fill's solves left it (p is what the assembly wrote).
int keep_info(VarCall &v, long long end) {
  if (v.reuse != 1) return CWBL_OK;
  int2 *const kept = v.cache->info.as<int2>();
  const long long n = std::min<long long>(end, v.cache->units) - v.win0;
  if (n <= 0) return CWBL_OK;
  HIPCHK(hipMemcpyAsync(kept + v.win0, S.info.p, (size_t)n * sizeof(int2),
                        hipMemcpyDeviceToDevice, S.stream));
  return CWBL_OK;
}

// build_tree of both families and the upload of their descriptors (nt = 0: nothing to do)
// Index mode 1, when a search first needs the trees: join the workers of the types that have
// one, upload the trees and the tree searches' descriptor table on stream s, raise max_depth.
// (A second table: the solves in flight keep reading S.tdesc.)
int ready_trees(VarCall &v, hipStream_t s) {
  if (v.trees_ready) return CWBL_OK;
  std::vector<TreeDesc> sd = v.descs;
  for (size_t i = 0; i < sd.size(); ++i) {
    TreeBufs *tb = v.tbs[i];
    if (!tb->worker_started) continue;  // cannot truncate: nodes stays null
    if (int rc = ready_tree(tb, s)) return rc;
    sd[i].nodes = tb->nodes.as<TreeNode>();
    sd[i].rdata = tb->rdata.as<float4>();
    sd[i].ind = tb->cell_order ? tb->ind2.as<int>() : tb->ind.as<int>();
    v.max_depth = std::max(v.max_depth, tb->depth);
  }
  HIPCHK(S.tdesc_tree.ensure(sd.size() * sizeof(TreeDesc)));
  // (from pageable memory: the copy has left `sd` when the call returns)
  HIPCHK(hipMemcpyAsync(S.tdesc_tree.p, sd.data(), sd.size() * sizeof(TreeDesc),
                        hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  v.trees_ready = true;
  return CWBL_OK;
}

int plan_trees(VarCall &v) {
  v.index1 = S.index_mode == 1;
  if (int rc = build_family(0, v.vp, v.descs, v.list_cap, v.max_depth, v.tbs)) return rc;
  if (int rc = build_family(1, v.vp, v.descs, v.list_cap, v.max_depth, v.tbs)) return rc;
  v.nt = (int)v.descs.size();
  IX.index_mode = S.index_mode;
  IX.types = v.nt;
  IX.cell_order = v.nt > 0 ? 1 : 0;
  for (const TreeBufs *tb : v.tbs)
    if (!tb->cell_order) IX.cell_order = 0;
  if (v.nt == 0 || v.npts == 0) return CWBL_OK;
  HIPCHK(S.tdesc.ensure(v.descs.size() * sizeof(TreeDesc)));
  HIPCHK(hipMemcpyAsync(S.tdesc.p, v.descs.data(), v.descs.size() * sizeof(TreeDesc),
                        hipMemcpyHostToDevice, S.stream));
  // the tree walk for every point needs every tree at once
  if (v.index1 && !S.binned)
    if (int rc = ready_trees(v, S.stream)) return rc;
  return CWBL_OK;
}

int stage_slab(VarCall &v) {
  const cwbl_slab *sl = v.sl;
  v.L = (long long)sl->nx * sl->ny * sl->nz;
  SlabDev &sd = v.sd;
  sd.nx = sl->nx; sd.ny = sl->ny; sd.nz = sl->nz; sd.alt_nx = sl->alt_nx;
  sd.alt_ny = sl->alt_ny; sd.ix_lim = sl->ix_lim; sd.iy_lim = sl->iy_lim; sd.L = v.L;
  const size_t bxy = (size_t)sl->nx * sl->ny * 4;
  const size_t balt = (size_t)sl->alt_nx * sl->alt_ny * sl->nz * 4;
  v.bvar = (size_t)v.L * S.k * 4;
  v.host = sl->memory != CWBL_MEM_DEVICE;
  // A group's host slabs move whole, from wherever they lie: not piped, page-locked or bounced.
  // So do a column-shared call's (its batches are columns, not contiguous runs of var).  Under
  // CWBL_OPT_HOST_PIPE both are piped like a single call's, when every var is page-locked or
  // can be for the call; they have no bounce-slot mode.
  const bool whole = v.group || v.colshare;
  const bool region = sl->ix_lim == sl->nx && sl->iy_lim == sl->ny;
  bool tune = false;
  for (int i = 0; i < v.nvar; ++i) tune = tune || v.vp[i].tune_q != 0;
  int reason = CWBL_TRANSFER_PIPED;
  if (!region) reason = CWBL_TRANSFER_REASON_REGION;
  else if (!S.host_pipe && (whole || tune)) reason = CWBL_TRANSFER_REASON_OFF;
  v.piped = v.host && region && (!whole || S.host_pipe);
  // pageable var (a Fortran host's ordinary arrays): copies from pageable memory are staged by
  // the runtime and do not overlap.  It is page-locked in place for the call (r4, C2 from
  // pageable numpy arrays: 58.7 M pts/s, against 58.2 M page-locked and 50.8 M through the
  // bounce slots, whose host copies stall the pipeline); the slots remain the fallback when
  // the registration fails (and CWBL_OPT_PAGEABLE = 1 forces them)
  v.bounce = !whole && v.host && v.bvar > 0 && !host_pinned(sl->var);
  if (v.bounce && S.pageable_register) {
    if (hipHostRegister(sl->var, v.bvar, hipHostRegisterDefault) == hipSuccess) {
      v.reg.push_back(sl->var);
      v.bounce = false;
    } else {
      (void)hipGetLastError();
    }
  }
  if (whole && v.piped && v.bvar > 0) {  // every var page-locked, or the call moves whole
    for (int i = 0; i < v.nvar && v.piped; ++i) {
      if (host_pinned(v.sl[i].var)) continue;
      if (!S.pageable_register) {
        reason = CWBL_TRANSFER_REASON_BOUNCE;
        v.piped = false;
      } else if (hipHostRegister(v.sl[i].var, v.bvar, hipHostRegisterDefault) == hipSuccess) {
        v.reg.push_back(v.sl[i].var);
      } else {
        (void)hipGetLastError();
        reason = CWBL_TRANSFER_REASON_REGISTER;
        v.piped = false;
      }
    }
    if (!v.piped) {  // undo the registrations made: whole moves take var from where it lies
      for (float *p : v.reg) (void)hipHostUnregister(p);
      v.reg.clear();
    }
  }
  v.registered = !v.reg.empty();
  // tune_q after the last batch touches the whole slab, so the analysis then goes back whole;
  // per batch (CWBL_OPT_HOST_PIPE) it leaves every batch final behind its own solve
  v.piped_back = v.piped && (!tune || S.host_pipe);
  v.tune_batch = v.piped_back && tune;
  TI.host = v.host;
  if (v.host) {
    TI.piped = v.piped;
    TI.piped_back = v.piped_back;
    TI.registered = (int)v.reg.size();
    TI.bounce = v.bounce;
    TI.reason = reason;
  }
  if (!v.host) {
    sd.x = sl->x; sd.y = sl->y; sd.alt = sl->alt;
    for (int i = 0; i < v.nvar; ++i) v.tv.var[i] = v.sl[i].var;
  } else {
    HIPCHK(stage(S.sx, sl->x, bxy, CWBL_MEM_HOST));
    HIPCHK(stage(S.sy, sl->y, bxy, CWBL_MEM_HOST));
    HIPCHK(stage(S.salt, sl->alt, balt, CWBL_MEM_HOST));
    sd.x = S.sx.as<float>(); sd.y = S.sy.as<float>(); sd.alt = S.salt.as<float>();
    // every variable has its own part of S.svar; var comes up here unless the batches pipe it
    // or stage_bounce moves it
    HIPCHK(S.svar.ensure(v.bvar * (size_t)v.nvar));
    for (int i = 0; i < v.nvar; ++i) {
      v.tv.var[i] = S.svar.as<float>() + (size_t)i * (size_t)v.L * S.k;
      if (v.bvar > 0 && !v.piped && !v.bounce) {
        HIPCHK(hipMemcpyAsync(v.tv.var[i], v.sl[i].var, v.bvar, hipMemcpyHostToDevice, S.stream));
        TI.bytes_whole_up += (long long)v.bvar;
      }
    }
  }
  sd.var = v.tv.var[0];
  return CWBL_OK;
}

void plan_batches(VarCall &v) {
  const long long npts = v.npts;
  const size_t per_pt = (size_t)v.list_cap * 4 + (size_t)v.nt * 4 + 8;
  long long B = (long long)(S.ws_bytes / per_pt);
  B = std::min<long long>(B, S.max_batch);
  // at least ~6 batches while they stay above 64 k points: with few batches the first search
  // and the last solve run alone (an 8-GPU rank's C2 share, 562 k points: 12.8 ms per step
  // in batches of 141 k, 12.3 in batches of 94 k; the full grid is indifferent in 100-160 k)
  if (!S.max_batch_set) B = std::min<long long>(B, std::max<long long>(npts / 6, 64000));
  B = std::max<long long>(std::min<long long>(B, npts), 256);
  B = std::min<long long>(B, 1 << 22);
  // a batch's lists stay below 4 GiB: search_binned_kernel addresses them by 32-bit offsets
  if (v.list_cap > 0)
    B = std::min<long long>(B, (long long)((((size_t)1 << 32) - 1) / ((size_t)v.list_cap * 4)) /
                                   kListLanes * kListLanes);
  // The first batch's search cannot overlap a solve, so it may be short (a lead of
  // 1/lead_div of the points); the rest are equal (a short last batch is all tail) and whole
  // list groups.
  const auto round_up = [](long long x) { return (x + kListLanes - 1) / kListLanes * kListLanes; };
  long long lead = S.lead_div > 0 ? round_up(npts / S.lead_div) : 0;
  if (lead < 4 * kListLanes || lead >= npts) lead = 0;
  if (lead > 0) v.plan.push_back({0, (int)std::min<long long>(lead, B)});
  const long long g1 = v.plan.empty() ? 0 : v.plan[0].second, rest = npts - g1;
  const long long nrest = (rest + B - 1) / B;
  const long long Br = round_up((rest + nrest - 1) / nrest);
  for (long long g = g1; g < npts; g += Br)
    v.plan.push_back({g, (int)std::min<long long>(Br, npts - g)});
  v.B = 0;
  for (const auto &b : v.plan) v.B = std::max<long long>(v.B, b.second);
  // bounce slots: one batch (or one whole-slab chunk of Bc points) of k member rows each
  v.Bc = std::min<long long>(std::max<long long>(v.B, 1), std::max<long long>(v.L, 1));
  // the per-point info of a window of up to S.info_window points is reduced once per window
  // (a reduction kernel per batch cost the C2 step ~0.5 ms)
  v.info_cap = std::max<long long>(v.B, std::min<long long>(npts, S.info_window));
}

// Whole-slab moves through the bounce slots (var not piped, or back after tune_q): chunk i of
// Bc points of every member row.  Up: fill slot i & 1 (once its copy two chunks back has left
// it), copy up on S.stream.  Down: copy chunk i down on S.stream, drain chunk i - 1 meanwhile.
int bounce_whole(VarCall &v, bool up) {
  std::vector<int> evs;
  long long pc0 = 0;
  int pcn = 0;
  const size_t pitch = (size_t)v.L * 4;
  float *const hvar = v.sl->var;
  (up ? TI.bytes_whole_up : TI.bytes_whole_down) += (long long)v.bvar;
  for (long long c0 = 0, i = 0; c0 < v.L; c0 += v.Bc, ++i) {
    const int cn = (int)std::min<long long>(v.Bc, v.L - c0);
    PinBuf &slot = up ? S.pin_in[i & 1] : S.pin_out[i & 1];
    hipEvent_t e;
    HIPCHK(cevent(v.cev, &e));
    if (up) {
      if (i >= 2) HIPCHK(hipEventSynchronize(S.cevents[evs[(size_t)i - 2]]));
      bounce_rows(S.pool, slot.as<float>(), hvar, v.L, c0, cn, S.k, true);
      HIPCHK(hipMemcpy2DAsync(S.svar.as<float>() + c0, pitch, slot.p, (size_t)cn * 4,
                              (size_t)cn * 4, (size_t)S.k, hipMemcpyHostToDevice, S.stream));
    } else {
      HIPCHK(hipMemcpy2DAsync(slot.p, (size_t)cn * 4, S.svar.as<float>() + c0, pitch,
                              (size_t)cn * 4, (size_t)S.k, hipMemcpyDeviceToHost, S.stream));
    }
    HIPCHK(hipEventRecord(e, S.stream));
    evs.push_back(v.cev++);
    if (!up && i >= 1) {
      HIPCHK(hipEventSynchronize(S.cevents[evs[(size_t)i - 1]]));
      bounce_rows(S.pool, S.pin_out[(i - 1) & 1].as<float>(), hvar, v.L, pc0, pcn, S.k, false);
    }
    pc0 = c0;
    pcn = cn;
  }
  if (!up && !evs.empty()) {
    HIPCHK(hipEventSynchronize(S.cevents[evs.back()]));
    bounce_rows(S.pool, S.pin_out[(evs.size() - 1) & 1].as<float>(), hvar, v.L, pc0, pcn,
                S.k, false);
  }
  return CWBL_OK;
}

// Piped bounce: batch b's columns into slot b % kSlots once the copy up of batch b - kSlots
// has left it; batch b's analysis out of its slot once its copy down is done.
int bounce_fill(VarCall &v, long long b) {
  if (b >= State::kSlots) HIPCHK(hipEventSynchronize(S.cevents[v.h2d_done[b - State::kSlots]]));
  bounce_rows(S.pool, S.pin_in[b % State::kSlots].as<float>(), v.sl->var, v.L, v.plan[b].first,
              v.plan[b].second, S.k, true);
  return CWBL_OK;
}

int bounce_drain(VarCall &v, long long b) {
  HIPCHK(hipEventSynchronize(S.cevents[v.d2h_done[b]]));
  bounce_rows(S.pool, S.pin_out[b % State::kSlots].as<float>(), v.sl->var, v.L, v.plan[b].first,
              v.plan[b].second, S.k, false);
  return CWBL_OK;
}

// The bounce slots of this call (page-locked only while a call needs them) and the whole-slab
// move up when var is not piped.
int stage_bounce(VarCall &v) {
  if (v.registered) {  // the slots are only the fallback's: give them back
    for (int i = 0; i < State::kSlots; ++i) {
      S.pin_in[i].release();
      S.pin_out[i].release();
    }
  }
  if (!v.bounce) return CWBL_OK;
  const size_t slot_bytes = (size_t)v.Bc * S.k * 4;
  const int nin = v.piped ? State::kSlots : 2, nout = v.piped_back ? State::kSlots : 2;
  for (int i = 0; i < nin; ++i) HIPCHK(S.pin_in[i].ensure(slot_bytes));
  for (int i = 0; i < nout; ++i) HIPCHK(S.pin_out[i].ensure(slot_bytes));
  if (!v.piped) return bounce_whole(v, true);
  return CWBL_OK;
}

// Per-call device buffers (two neighbour-list buffers: the search of batch b + 1 overlaps the
// solve of batch b) and the solve constants.
int alloc_call_buffers(VarCall &v) {
  const long long B = v.B;
  const size_t bytes_cnt = (size_t)B * v.nt * 4;
  const size_t bytes_idx =
      (size_t)((B + kListLanes - 1) / kListLanes) * kListLanes * std::max(v.list_cap, 1) * 4;
  HIPCHK(S.nbr_cnt.ensure(bytes_cnt));
  HIPCHK(S.nbr_idx.ensure(bytes_idx));
  if (v.plan.size() > 1) {
    HIPCHK(S.nbr_cnt2.ensure(bytes_cnt));
    HIPCHK(S.nbr_idx2.ensure(bytes_idx));
  }
  HIPCHK(S.flags.ensure((size_t)(B + 1) * sizeof(int)));
  HIPCHK(S.stats.ensure(sizeof(DevStats)));
  HIPCHK(hipMemsetAsync(S.stats.p, 0, sizeof(DevStats), S.stream));
  HIPCHK(S.info.ensure((size_t)v.info_cap * sizeof(int2)));
  v.c = solve_consts((float)(S.k - 1) / v.vp->multi_infl,  // inflat (:68)
                     v.vp->use_rtpp, v.vp->rtpp_alpha, v.vp->use_rtps, v.vp->rtps_alpha);
  v.c.ntrees = v.nt;
  v.c.list_cap = v.list_cap;
  // bounding-box half-width of the binned search: the radius with a margin, so that every
  // point with d2 <= r2 in fp32 lies inside
  v.rbox = std::sqrt(search_r2()) * 1.0001f + 1e-5f;
  return CWBL_OK;
}

// get_lz for every point of batch bi (module_localization.f90:188-331) on S.sstream: uniform
// bins, then the k-d tree walk for the points whose lists pass max_lz_pts (Q4); or the tree
// walk for every point (CWBL_OPT_SEARCH = 1).  Waits for the solve two batches back, which
// read the same list buffer.
int search_batch(VarCall &v, long long bi, int *ncnt, int *nidx, hipEvent_t a, hipEvent_t b) {
  const long long g0 = v.plan[bi].first;
  const int nb = v.plan[bi].second;
  const TreeDesc *dtrees = S.tdesc.as<TreeDesc>();
  DevStats *dst = S.stats.as<DevStats>();
  // (timing experiment: CWBL_DEBUG_SERIAL=1 runs the searches on the solve stream)
  hipStream_t ss = S.serial_search ? S.stream : S.sstream;
  // (no event yet: the search of the first batch past the cached ones, queued ahead of the
  // merged hit launch that covers batch bi - 2, which reads no lists)
  if (bi >= 2 && bi - 2 < (long long)v.done_ev.size())
    HIPCHK(hipStreamWaitEvent(ss, S.events[v.done_ev[bi - 2]], 0));
  HIPCHK(hipEventRecord(a, ss));
  int kt;
  if (S.binned) {
    int *fcnt = S.flags.as<int>(), *fidx = fcnt + 1;
    HIPCHK(hipMemsetAsync(fcnt, 0, sizeof(int), ss));
    HIPCHK(kt_begin(ss, &kt));
    HIPCHK(launch_search_binned(ss, dtrees, v.nt, v.list_cap, v.c.r2, v.rbox, v.sd, g0, nb, ncnt,
                                nidx, fcnt, fidx));
    HIPCHK(kt_end(ss, kt, KT_SEARCH_BINNED, nb));
    if (v.index1) {
      // the batch's flag count, waited for on the search stream only (the previous batch's
      // solve is already queued on S.stream): no flagged point, no tree search and no tree
      HIPCHK(S.ix_pin.ensure(64));
      int *hcnt = S.ix_pin.as<int>();
      HIPCHK(hipMemcpyAsync(hcnt, fcnt, sizeof(int), hipMemcpyDeviceToHost, ss));
      HIPCHK(hipStreamSynchronize(ss));
      if (*hcnt > 0) {
        ++P.flagged_batches;
        if (int rc = ready_trees(v, ss)) return rc;
        HIPCHK(kt_begin(ss, &kt));
        HIPCHK(launch_search_flagged(ss, S.tdesc_tree.as<TreeDesc>(), v.nt, v.max_depth,
                                     v.list_cap, v.c.r2, v.sd, g0, nb, fcnt, fidx, ncnt, nidx,
                                     dst, true));
        HIPCHK(kt_end(ss, kt, KT_SEARCH_FLAGGED, 0));
      }
    } else {
      HIPCHK(kt_begin(ss, &kt));
      HIPCHK(launch_search_flagged(ss, dtrees, v.nt, v.max_depth, v.list_cap, v.c.r2, v.sd, g0,
                                   nb, fcnt, fidx, ncnt, nidx, dst));
      HIPCHK(kt_end(ss, kt, KT_SEARCH_FLAGGED, 0));
    }
  } else if (v.index1) {
    HIPCHK(kt_begin(ss, &kt));
    HIPCHK(launch_search(ss, S.tdesc_tree.as<TreeDesc>(), v.nt, v.max_depth, v.list_cap, v.c.r2,
                         v.sd, g0, nb, ncnt, nidx, nullptr, dst, true));
    HIPCHK(kt_end(ss, kt, KT_SEARCH_TREE, nb));
  } else {
    HIPCHK(kt_begin(ss, &kt));
    HIPCHK(launch_search(ss, dtrees, v.nt, v.max_depth, v.list_cap, v.c.r2, v.sd, g0, nb, ncnt,
                         nidx, nullptr, dst));
    HIPCHK(kt_end(ss, kt, KT_SEARCH_TREE, nb));
  }
  return hipEventRecord(b, ss) == hipSuccess ? CWBL_OK
                                              : fail(CWBL_ERR_HIP, "search event record failed");
}

// The rows of batch bi in a host slab's var and in its staged copy: k rows of nb floats at the
// member pitch L per variable, variable i at its part of S.svar; for a column-shared call, whose
// batch is the columns [g0, g0 + nb), nz k rows at the plane pitch nx ny (a column run is
// contiguous in every (level, member) plane).  One 2-D copy per variable either way.
struct BatchRows {
  size_t pitch, rows, width;
};
BatchRows batch_rows(const VarCall &v, int nb) {
  if (v.colshare)
    return {(size_t)v.sl->nx * v.sl->ny * 4, (size_t)v.sl->nz * S.k, (size_t)nb * 4};
  return {(size_t)v.L * 4, (size_t)S.k, (size_t)nb * 4};
}

// A host slab's var columns of batch bi up on S.h2d, from the caller's page-locked arrays (a
// group: every variable's, then one event) or from the batch's bounce slot; S.stream waits.
int upload_batch_var(VarCall &v, long long bi) {
  const long long g0 = v.plan[bi].first;
  const int nb = v.plan[bi].second;
  hipEvent_t hv;
  const int hv_i = v.cev++;
  HIPCHK(cevent(hv_i, &hv));
  const BatchRows r = batch_rows(v, nb);
  if (v.bounce) {  // slot bi % kSlots, filled before this batch (bounce_fill)
    if (bi == 0)
      if (int rc = bounce_fill(v, 0)) return rc;
    HIPCHK(hipMemcpy2DAsync(S.svar.as<float>() + g0, r.pitch, S.pin_in[bi % State::kSlots].p,
                            r.width, r.width, r.rows, hipMemcpyHostToDevice, S.h2d));
  } else {
    for (int i = 0; i < v.nvar; ++i)
      HIPCHK(hipMemcpy2DAsync(S.svar.as<float>() + (size_t)i * (size_t)v.L * S.k + g0, r.pitch,
                              v.sl[i].var + g0, r.pitch, r.width, r.rows, hipMemcpyHostToDevice,
                              S.h2d));
  }
  TI.bytes_piped_up += (long long)(r.width * r.rows) * v.nvar;
  HIPCHK(hipEventRecord(hv, S.h2d));
  v.h2d_done.push_back(hv_i);
  HIPCHK(hipStreamWaitEvent(S.stream, hv, 0));
  return CWBL_OK;
}

// Batch bi's analysis back to a host slab on S.d2h behind the event dn: the one after its
// solve, or after its tune_q (tune_batch_var).
int return_batch_var(VarCall &v, long long bi, hipEvent_t dn) {
  const long long g0 = v.plan[bi].first;
  const int nb = v.plan[bi].second;
  HIPCHK(hipStreamWaitEvent(S.d2h, dn, 0));
  const BatchRows r = batch_rows(v, nb);
  if (v.bounce) {  // into slot bi % kSlots (drained kSlots - 1 batches later)
    hipEvent_t dv;
    const int dv_i = v.cev++;
    HIPCHK(cevent(dv_i, &dv));
    HIPCHK(hipMemcpy2DAsync(S.pin_out[bi % State::kSlots].p, r.width, S.svar.as<float>() + g0,
                            r.pitch, r.width, r.rows, hipMemcpyDeviceToHost, S.d2h));
    HIPCHK(hipEventRecord(dv, S.d2h));
    v.d2h_done.push_back(dv_i);
  } else {
    for (int i = 0; i < v.nvar; ++i)
      HIPCHK(hipMemcpy2DAsync(v.sl[i].var + g0, r.pitch,
                              S.svar.as<float>() + (size_t)i * (size_t)v.L * S.k + g0, r.pitch,
                              r.width, r.rows, hipMemcpyDeviceToHost, S.d2h));
  }
  TI.bytes_piped_down += (long long)(r.width * r.rows) * v.nvar;
  return CWBL_OK;
}

// letkf_tune_q over batch (g0, nb) on S.stream, for the variables that ask for it: the batch's
// points, or for a column-shared call its columns at every level.  The kernel is pointwise
// (each point reads and writes only its own k members), and the batches of a piped call cover
// every point of the slab, the ones the solve skips (p = 0) included.
int tune_batch_var(VarCall &v, long long g0, int nb) {
  for (int i = 0; i < v.nvar; ++i) {
    if (!v.vp[i].tune_q) continue;
    SlabDev sdi = v.colshare ? v.full : v.sd;  // (a shared call: the slab, not its column view)
    sdi.var = S.svar.as<float>() + (size_t)i * (size_t)v.L * S.k;
    int kt;
    HIPCHK(kt_begin(S.stream, &kt));
    HIPCHK(launch_tune_q_range(S.stream, sdi, S.k, g0, nb, v.nlev, v.colshare ? v.ncol : 0));
    HIPCHK(kt_end(S.stream, kt, KT_TUNE_Q, (long long)nb * v.nlev));
    ++TI.tune_q_launches;
  }
  return CWBL_OK;
}

// Sub-batches of a search batch for a path with a per-point record: ns points (a multiple of
// kListLanes, so a sub-batch's neighbour lists start on a list group) with at most `cap`
// points each, the batch split evenly.
long long sub_batch(int nb, long long cap) {
  const long long nsub = (nb + cap - 1) / cap;
  const long long Bs = (nb + nsub - 1) / nsub;
  return std::max<long long>(kListLanes, (Bs + kListLanes - 1) / kListLanes * kListLanes);
}
// The record path's sub-batch: CWBL_OPT_SPLIT40_BATCH, and at most 2^19 points (the solve
// addresses a sub-batch's records with 32-bit byte offsets).  A merged hit's segments are these.
long long record_sub_batch(int nb) {
  const long long cap = std::min<long long>(S.tq4_sub > 0 ? S.tq4_sub : nb, 1 << 19);
  return std::min<long long>(sub_batch(nb, cap), 1 << 19);
}
// The hand-off path's sub-batch of a call of nv variables: CWBL_OPT_BIG_BATCH, and what the
// hand-off budget holds of its records (cwbl_init: workspace_bytes when the caller gave one,
// else 13 GB or 40% of the free device memory).  BigHandoff<128, 64> is 134.7 KB per point:
// 13 GB at the default 98 304-point sub-batch, outside workspace_bytes.
long long handoff_sub_batch(int nb, int nv) {
  const size_t rec_bytes = 8 * big_handoff_words(S.kp, nv);
  const long long fit = std::max<long long>(
      kListLanes, (long long)(S.handoff_budget / rec_bytes) / kListLanes * kListLanes);
  return sub_batch(nb, std::min<long long>(S.big_sub, fit));
}

// letkf_yoyb + letkf_solve (module_letkf_core.f90:300-700) for batch (g0, nb) on S.stream, one
// path per ensemble-size class:
//   k = 17..40   record path: assemble_record_kernel -> record -> solve_tq40_kernel, or
//                solve_tq40_multi_kernel for a group call
//   k = 65..128  hand-off path: 256-thread kernel (assembly + first steps) -> record ->
//                solve_tqb_tail_kernel, or the group forms of the two for a group call;
//                CWBL_OPT_BIG_PATH = 0: one 256-thread kernel
//   otherwise    one wavefront per point: solve_tq_kernel, or solve_tq_multi_kernel for a
//                group call; CWBL_OPT_SOLVER = 1: the Jacobi eigensolver kernel (k <= 64)
// b2 / dn: the events around the batch's solve (the record path times its kernel pair
// between them).  crec: a cached batch's region of the record cache (every sub-batch's), in
// the call's form (the table above CacheForm; None with a null crec), which a fill (hit false)
// writes and a hit (no lists, no trees) solves from.  Record path: a fill assembles into crec
// in S.wsa's place; caux is the region's FactorAux entries (Tq40Factor; else null and unused).
// One-wavefront path: a fill runs fill_tq_wave_kernel in solve_tq_kernel's place.  Hand-off
// path: a fill runs fill_tqb_tail_kernel in the tail's place, a hit no hand-off kernel.
int solve_batch_path(VarCall &v, long long g0, int nb, const int *ncnt, const int *nidx,
                     int2 *infob, hipEvent_t b2, hipEvent_t dn, double *crec = nullptr,
                     CacheForm form = CacheForm::None, bool hit = false, double *caux = nullptr) {
  const TreeDesc *dtrees = S.tdesc.as<TreeDesc>();
  const SolveConsts &c = v.c;
  const SlabDev &sd = v.sd;
  const int nt = v.nt, list_cap = v.list_cap;
  int kt;
  const bool handoff = handoff_path();
  if (record_path()) {
    const long long Bs = record_sub_batch(nb);
    // (+1: the spare record of solve_tq40_kernel's lanes past the sub-batch)
    if (!crec) HIPCHK(S.wsa.ensure((size_t)(Bs + 1) * 8 * AsmRecord<kTq4KP>::WORDS));
    double *rec = crec ? crec : S.wsa.as<double>();
    // a cached batch keeps every sub-batch's records, S.wsa only the current one's
    const size_t rstep = crec ? AsmRecord<kTq4KP>::WORDS : 0;
    // the solve of n points from g: one variable's, or the group's over all its variables
    // A cached batch of factors: its fill's solve leaves the factor over each record.  (A group
    // call never has a cached batch.)
    const bool factor = form == CacheForm::Tq40Factor;
    const int kt_solve = factor ? (hit ? KT_SOLVE_TQ40_FACTOR : KT_FILL_TQ40_FACTOR)
                         : v.group ? KT_SOLVE_TQ40_MULTI : KT_SOLVE_TQ40;
    auto solve = [&](long long g, int n, double *r, int2 *inf) {
      if (factor) {
        // (the entries of the records r: the same ordinal within the batch's region)
        double *const ax = caux + (size_t)(r - rec) / rstep * FactorAux<kTq4KP>::WORDS;
        return hit ? launch_solve_tq40_factor(S.stream, S.kp, c, sd, g, n, r, ax, inf)
                   : launch_fill_tq40_factor(S.stream, S.kp, c, sd, g, n, r, ax, inf);
      }
      return v.group ? launch_solve_tq40_multi(S.stream, S.kp, c, sd, v.tv, g, n, r, inf)
                     : launch_solve_tq40(S.stream, S.kp, c, sd, g, n, r, inf);
    };
    if (Bs >= nb && hit) {
      if (S.ktiming) S.kpend.push_back({kt_solve, b2, dn, nb});
      HIPCHK(solve(g0, nb, rec, infob));
      return CWBL_OK;
    }
    if (Bs >= nb) {  // the whole batch: timed between b2 and dn (recorded anyway)
      auto asm_ = [&]() {
        return launch_assemble_record(S.stream, S.kp, dtrees, c, sd, g0, nb, ncnt, nidx, infob,
                                      rec);
      };
      auto tq40 = [&]() { return solve(g0, nb, rec, infob); };
      HIPCHK(kt_pair(S.stream, b2, KT_ASSEMBLE_RECORD, nb, dn, kt_solve, nb, asm_, tq40));
      return CWBL_OK;
    }
    for (long long s0 = 0; s0 < nb; s0 += Bs) {
      const int ns = (int)std::min<long long>(Bs, nb - s0);
      double *const srec = rec + (size_t)s0 * rstep;
      if (!hit) {
        HIPCHK(kt_begin(S.stream, &kt));
        HIPCHK(launch_assemble_record(S.stream, S.kp, dtrees, c, sd, g0 + s0, ns,
                                      ncnt + s0 * nt, nidx + s0 * list_cap, infob + s0, srec));
        HIPCHK(kt_end(S.stream, kt, KT_ASSEMBLE_RECORD, ns));
      }
      HIPCHK(kt_begin(S.stream, &kt));
      HIPCHK(solve(g0 + s0, ns, srec, infob + s0));
      HIPCHK(kt_end(S.stream, kt, kt_solve, ns));
    }
    return CWBL_OK;
  }
  if (handoff) {
    // (a group's record carries the further variables' Q^T x': BigHandoffMulti)
    const int nv = v.group ? group_var_class(v.nvar) : 1;
    const size_t rec_bytes = 8 * big_handoff_words(S.kp, nv);
    const int ci = nv == 2 ? 0 : nv == 4 ? 1 : 2;  // the group kernels' KernelId offset
    const long long Bs = handoff_sub_batch(nb, nv);
    // a cached batch of the factor cache: sub-batch s0 starts s0 factors into its region
    const bool bigf = form == CacheForm::BigFactor;
    const size_t fwords = big_factor_words(S.kp);
    if (!(bigf && hit)) HIPCHK(S.wsa.ensure((size_t)Bs * rec_bytes));
    for (long long s0 = 0; s0 < nb; s0 += Bs) {
      const int ns = (int)std::min<long long>(Bs, nb - s0);
      HIPCHK(kt_begin(S.stream, &kt));
      if (bigf && hit) {
        HIPCHK(launch_solve_tqb_factor(S.stream, S.kp, c, sd, g0 + s0, ns,
                                       crec + (size_t)s0 * fwords, infob + s0));
        HIPCHK(kt_end(S.stream, kt, KT_SOLVE_TQB_FACTOR, ns));
        continue;
      }
      if (v.group) {
        HIPCHK(launch_big_handoff_multi(S.stream, S.kp, dtrees, c, sd, v.tv, g0 + s0, ns,
                                        ncnt + s0 * nt, nidx + s0 * list_cap, infob + s0,
                                        S.wsa.as<double>()));
        HIPCHK(kt_end(S.stream, kt, KT_BIG_HANDOFF_MULTI2 + ci, (long long)ns * v.lev));
        HIPCHK(kt_begin(S.stream, &kt));
        HIPCHK(launch_solve_tqb_tail_multi(S.stream, S.kp, c, sd, v.tv, g0 + s0, ns,
                                           S.wsa.as<double>(), infob + s0));
        HIPCHK(kt_end(S.stream, kt, KT_TQB_TAIL_MULTI2 + ci, (long long)ns * v.lev));
        continue;
      }
      HIPCHK(launch_big_handoff(S.stream, S.kp, dtrees, c, sd, g0 + s0, ns, ncnt + s0 * nt,
                                nidx + s0 * list_cap, infob + s0, S.wsa.as<double>()));
      HIPCHK(kt_end(S.stream, kt, KT_BIG_HANDOFF, ns));
      HIPCHK(kt_begin(S.stream, &kt));
      if (bigf) {
        HIPCHK(launch_fill_tqb_tail(S.stream, S.kp, c, sd, g0 + s0, ns, S.wsa.as<double>(),
                                    infob + s0, crec + (size_t)s0 * fwords));
        HIPCHK(kt_end(S.stream, kt, KT_FILL_TQB_TAIL, ns));
        continue;
      }
      HIPCHK(launch_solve_tqb_tail(S.stream, S.kp, c, sd, g0 + s0, ns, S.wsa.as<double>(),
                                   infob + s0));
      HIPCHK(kt_end(S.stream, kt, KT_TQB_TAIL, ns));
    }
    return CWBL_OK;
  }
  HIPCHK(kt_begin(S.stream, &kt));
  if (S.kp > kMaxWaveKP) {
    HIPCHK(launch_solve_tq_big(S.stream, S.kp, false, dtrees, c, sd, g0, nb, ncnt, nidx,
                               nullptr, nullptr, nullptr, nullptr, nullptr, infob));
    HIPCHK(kt_end(S.stream, kt, KT_SOLVE_TQ_BIG, nb));
  } else if (S.jacobi) {
    HIPCHK(launch_solve_neighbors(S.stream, S.kp, dtrees, c, sd, g0, nb, ncnt, nidx, infob));
    HIPCHK(kt_end(S.stream, kt, KT_SOLVE_JACOBI, nb));
  } else if (v.group) {
    HIPCHK(launch_solve_tq_multi(S.stream, S.kp, dtrees, c, sd, v.tv, g0, nb, ncnt, nidx, infob));
    const int nv = group_var_class(v.nvar);
    HIPCHK(kt_end(S.stream, kt, nv == 2 ? KT_SOLVE_TQ_MULTI2 : nv == 4 ? KT_SOLVE_TQ_MULTI4
                                                                      : KT_SOLVE_TQ_MULTI8,
                  (long long)nb * v.lev));
  } else if (form == CacheForm::WaveFactor) {  // a cached batch (CWBL_OPT_WAVE_REUSE)
    if (hit) {
      HIPCHK(launch_solve_tq_wave_factor(S.stream, S.kp, c, sd, g0, nb, crec, infob));
    } else {
      HIPCHK(launch_fill_tq_wave(S.stream, S.kp, dtrees, c, sd, g0, nb, ncnt, nidx, infob, crec));
    }
    HIPCHK(kt_end(S.stream, kt, hit ? KT_SOLVE_TQ_WAVE_FACTOR : KT_FILL_TQ_WAVE, nb));
  } else {
    HIPCHK(launch_solve_tq(S.stream, S.kp, false, dtrees, c, sd, g0, nb, ncnt, nidx, nullptr,
                           nullptr, nullptr, nullptr, nullptr, infob));
    HIPCHK(kt_end(S.stream, kt, KT_SOLVE_TQ, nb));
  }
  return CWBL_OK;
}

// The hand-off path's classes whose shared calls solve every level from one kept factor per
// column: KP = 96, and KP = 128 (k = 97..128) where CWBL_OPT_COLUMN_ROWS admits it.  The option
// does nothing on its own (CWBL_OPT_COLUMN_FACTOR or CWBL_OPT_COLUMN_REUSE has to be set) and is
// accepted and ignored at the other KP and on every other path.
bool handoff_column_path() {
  return handoff_path() && (S.kp == 96 || (S.kp == kBigSplitKP && S.column_rows));
}

// ---- CWBL_OPT_COLUMN_REUSE ---------------------------------------------------------------------
// The classes whose column-shared calls fill and read the column cache: the paths with a
// per-column form and a kernel that solves every level from it.  Accepted and ignored elsewhere
// (k <= 16, CWBL_OPT_SPLIT40 = 0, CWBL_OPT_SOLVER = 1, CWBL_OPT_BIG_PATH = 0, k = 97..128; the
// last is served under CWBL_OPT_COLUMN_ROWS = 1).
bool column_reuse_path() {
  return S.column_reuse > 0 && S.column_share != 0 &&
         (record_path() || (wave_path() && S.kp > kTq4KP) || handoff_column_path());
}
CacheForm column_form() {
  return record_path() ? CacheForm::Records
         : wave_path() ? CacheForm::WaveFactor
                       : CacheForm::BigFactor;
}

// ---- CWBL_OPT_COLUMN_SHARE ---------------------------------------------------------------------
// Why a call of one variable does not run once per column, from what is known before the
// trees are planned (CWBL_COLUMN_SHARED: it may).  The type rule restates build_family's
// selection: with no used type of vclr > 0 every tree is 2-D, queried in 2-D and outside the
// Q1 undefined case; analyze_call checks the planned descriptors themselves afterwards.
int column_reason(const VarCall &v) {
  if (!S.column_share) return CWBL_COLUMN_REASON_OFF;
  if (v.nvar > 1) return CWBL_COLUMN_REASON_GROUP;
  // (where the column cache serves, a call of one level is shared too: it fills or hits)
  if (v.sl->nz < (column_reuse_path() ? 1 : 2)) return CWBL_COLUMN_REASON_NZ;
  if (!(record_path() || wave_path() || handoff_path())) return CWBL_COLUMN_REASON_PATH;
  for (const ObsType &ot : S.obs) {
    if (ot.nobs <= 0 || (ot.family == 0 && !is_gts_assimilated(ot.type_id))) continue;
    const cwbl_type_params &tp =
        ot.family == 0 ? v.vp->gts[ot.type_id - 1] : v.vp->radar[ot.type_id - 1];
    if (tp.use_it && tp.hclr > 0.0f && tp.vclr > 0.0f) return CWBL_COLUMN_REASON_3D;
  }
  return CWBL_COLUMN_SHARED;
}

// Levels per wavefront of a solve_tq40_column_kernel launch over ncol columns: the option, or
// all nz unless the columns' waves are fewer than twice what the device holds of this kernel
// (two waves per SIMD); then the fewest level ranges that reach that many waves.
int column_levels_per_wave(int ncol, int nz) {
  int lw = nz;
  if (S.column_levels > 0) {
    lw = std::min(S.column_levels, nz);
  } else {
    const long long waves = (ncol + 3) / 4, want = 2LL * S.ncu * 4 * 2;
    if (waves < want) {
      const long long ranges = std::min<long long>(nz, (want + waves - 1) / waves);
      lw = (int)((nz + ranges - 1) / ranges);
    }
  }
  return std::max(lw, (nz + 65534) / 65535);  // gridDim.y
}

// CWBL_OPT_COLUMN_FACTOR: a shared call's levels from one kept factor per column, where the
// path has a factor form with a fill and a hit kernel and the level kernel met its bar
// (DESIGN.md §3.6): the one-wavefront path at KP = 48, 56, 64 and the hand-off path at KP = 96.
// Accepted and ignored elsewhere (k <= 40, k = 97..128; the last is served under
// CWBL_OPT_COLUMN_ROWS = 1).
bool column_factor_path() {
  return S.column_factor && ((wave_path() && S.kp > kTq4KP) || handoff_column_path());
}

// Levels per wavefront of a level kernel's launch over ncol columns and the nl = nz - 1 levels
// above level 0, one column per wavefront: the option, or all nl unless the columns are fewer
// than twice the wavefronts the device holds of the kernel (TqOccupancy per SIMD: three at
// KP = 48, two at every other KP, KP = 128 among them); then the fewest level ranges that reach
// that many.
int factor_levels_per_wave(int ncol, int nl) {
  int lw = nl;
  if (S.column_levels > 0) {
    lw = std::min(S.column_levels, nl);
  } else {
    const long long want = 2LL * S.ncu * 4 * (S.kp == 48 ? 3 : 2);
    if (ncol < want) {
      const long long ranges = std::min<long long>(nl, (want + ncol - 1) / ncol);
      lw = (int)((nl + ranges - 1) / ranges);
    }
  }
  return std::max(lw, (nl + 65534) / 65535);  // gridDim.y
}

// The solves of batch (g0, nb) of a column-shared call under CWBL_OPT_COLUMN_FACTOR (v.sd is the
// column view, v.full the slab).  Per (sub-)batch of ns columns: the factor cache's fill on the
// column view analyses level 0 as the single kernels do and leaves the ns factors in S.wsf, a
// workspace of the call; one launch of the level kernel then solves the levels 1 .. nz-1 of
// every column from them.  The record cache is not involved.  done = false (and nothing
// launched) when the workspace cannot be allocated: the caller runs the chunks, no error.
// crec: a cached batch's region of the column cache (CWBL_OPT_COLUMN_REUSE), the factors' place
// instead of S.wsf, sub-batch s0 starting s0 factors in.  A fill (hit false) runs as above; a hit
// runs no hand-off kernel and no fill, and one launch of the all-levels kernel per (sub-)batch
// solves the levels 0 .. nz-1 from the kept factors.
int solve_batch_column_factor(VarCall &v, long long g0, int nb, const int *ncnt, const int *nidx,
                              int2 *infob, bool &done, double *crec = nullptr, bool hit = false) {
  const TreeDesc *dtrees = S.tdesc.as<TreeDesc>();
  const SolveConsts &c = v.c;
  const int nz = v.nlev, nt = v.nt, list_cap = v.list_cap;
  const bool handoff = handoff_path();
  const size_t fwords = handoff ? big_factor_words(S.kp) : wave_factor_words(S.kp);
  const size_t rec_bytes = handoff ? 8 * big_handoff_words(S.kp, 1) : 0;
  const long long Bs = handoff ? handoff_sub_batch(nb, 1) : nb;  // (solve_batch_path's)
  // (+1: the spare entry, as the record cache's regions have one)
  if (!crec &&
      S.wsf.ensure((size_t)(std::min<long long>(Bs, nb) + 1) * fwords * 8) != hipSuccess) {
    (void)hipGetLastError();
    CI.from_factor = 0;
    CI.levels_per_wave = 0;
    done = false;
    return CWBL_OK;
  }
  if (handoff && !hit) HIPCHK(S.wsa.ensure((size_t)Bs * rec_bytes));
  int kt;
  for (long long s0 = 0; s0 < nb; s0 += Bs) {
    const int ns = (int)std::min<long long>(Bs, nb - s0);
    int2 *const inf = infob + s0;
    double *const fac = crec ? crec + (size_t)s0 * fwords : S.wsf.as<double>();
    HIPCHK(kt_begin(S.stream, &kt));
    if (hit) {
      const int lw = factor_levels_per_wave(ns, nz);
      CI.levels_per_wave = lw;
      if (handoff)
        HIPCHK(launch_solve_tqb_factor_column_all(S.stream, S.kp, c, v.full, g0 + s0, ns, nz, lw,
                                                  fac, inf));
      else
        HIPCHK(launch_solve_tq_wave_factor_column_all(S.stream, S.kp, c, v.full, g0 + s0, ns, nz,
                                                      lw, fac, inf));
      HIPCHK(kt_end(S.stream, kt,
                    handoff ? KT_SOLVE_TQB_FACTOR_COLUMN_ALL : KT_SOLVE_TQ_WAVE_FACTOR_COLUMN_ALL,
                    (long long)ns * nz));
      continue;
    }
    if (handoff) {
      HIPCHK(launch_big_handoff(S.stream, S.kp, dtrees, c, v.sd, g0 + s0, ns, ncnt + s0 * nt,
                                nidx + s0 * list_cap, inf, S.wsa.as<double>()));
      HIPCHK(kt_end(S.stream, kt, KT_BIG_HANDOFF, ns));
      HIPCHK(kt_begin(S.stream, &kt));
      HIPCHK(launch_fill_tqb_tail(S.stream, S.kp, c, v.sd, g0 + s0, ns, S.wsa.as<double>(), inf,
                                  fac));
      HIPCHK(kt_end(S.stream, kt, KT_FILL_TQB_TAIL, ns));
    } else {
      HIPCHK(launch_fill_tq_wave(S.stream, S.kp, dtrees, c, v.sd, g0 + s0, ns, ncnt + s0 * nt,
                                 nidx + s0 * list_cap, inf, fac));
      HIPCHK(kt_end(S.stream, kt, KT_FILL_TQ_WAVE, ns));
    }
    if (nz < 2) {  // (a call of one level, CWBL_OPT_COLUMN_REUSE: the fill was all of it)
      CI.levels_per_wave = 0;
      continue;
    }
    const int lw = factor_levels_per_wave(ns, nz - 1);
    CI.levels_per_wave = lw;
    HIPCHK(kt_begin(S.stream, &kt));
    if (handoff)
      HIPCHK(launch_solve_tqb_factor_column(S.stream, S.kp, c, v.full, g0 + s0, ns, nz, lw, fac,
                                            inf));
    else
      HIPCHK(launch_solve_tq_wave_factor_column(S.stream, S.kp, c, v.full, g0 + s0, ns, nz, lw,
                                                fac, inf));
    HIPCHK(kt_end(S.stream, kt,
                  handoff ? KT_SOLVE_TQB_FACTOR_COLUMN : KT_SOLVE_TQ_WAVE_FACTOR_COLUMN,
                  (long long)ns * (nz - 1)));
  }
  CI.from_factor = 1;
  CI.chunk_launches = 0;
  done = true;
  return CWBL_OK;
}

// The solves of batch (g0, nb) of a column-shared call: g0 and nb count columns, the lists and
// infob are the columns'.
//   record path, option 1   assemble_record_kernel over the columns as it is, then
//                           solve_tq40_column_kernel over the same records with the whole slab
//   CWBL_OPT_COLUMN_FACTOR  (either option at k = 41..96, and at k = 97..128 under
//                           CWBL_OPT_COLUMN_ROWS) solve_batch_column_factor above; the
//                           chunks below only if its workspace cannot be allocated
//   chunked paths           (option 1 elsewhere, option 2 everywhere) the levels in chunks of up
//                           to kMaxGroupVars: each chunk is the path's group launch on the column
//                           view with var[i] = var + (kz0 + i) nx ny and the call's flags for
//                           every level; a remainder of one level runs the single kernel with
//                           sd.var offset likewise.  The batch's lists, and on the record path
//                           its records, serve every chunk.
// crec / hit: a cached batch's region of the column cache (CWBL_OPT_COLUMN_REUSE).  Such a batch
// always runs the one-factor form, whatever the two options say: on the record path the
// assembly straight into the region and solve_tq40_column_kernel, a hit the latter alone; above
// k = 40 solve_batch_column_factor on the region.
int solve_batch_column(VarCall &v, long long g0, int nb, const int *ncnt, const int *nidx,
                       int2 *infob, hipEvent_t b2, hipEvent_t dn, double *crec = nullptr,
                       bool hit = false) {
  const int nz = v.nlev;
  const long long nxy = (long long)v.full.nx * v.full.ny;
  float *const var0 = v.full.var;
  // the view of levels kz0 .. kz0 + n - 1 as a group of n variables (n = 1: a single call)
  auto chunk = [&](int kz0, int n) {
    v.sd.var = var0 + nxy * kz0;
    v.group = n > 1;
    v.nvar = n;
    v.lev = n;
    v.tv.nvar = n;
    for (int i = 0; i < n; ++i) {
      v.tv.var[i] = var0 + nxy * (kz0 + i);
      v.tv.use_rtpp[i] = v.vp->use_rtpp;
      v.tv.use_rtps[i] = v.vp->use_rtps;
      v.tv.rtpp_alpha[i] = v.vp->rtpp_alpha;
      v.tv.rtps_alpha[i] = v.vp->rtps_alpha;
    }
  };
  // the call's own view again, on every return path (finish_call reads tv.var[0])
  struct Restore {
    VarCall &v;
    Tq40Vars tv;
    SlabDev sd;
    bool group;
    ~Restore() {
      v.tv = tv;
      v.sd = sd;
      v.group = group;
      v.nvar = 1;
      v.lev = 1;
    }
  } restore{v, v.tv, v.sd, v.group};
  if (column_factor_path() || (crec && !record_path())) {
    bool done = false;
    if (int rc = solve_batch_column_factor(v, g0, nb, ncnt, nidx, infob, done, crec, hit))
      return rc;
    if (done) return CWBL_OK;  // (else: no workspace, the chunks below)
  }
  const bool column_kernel = v.colshare == 1 || crec;
  CI.chunk_launches = column_kernel && record_path() ? 0 : (nz + kMaxGroupVars - 1) / kMaxGroupVars;
  if (!record_path()) {
    for (int kz0 = 0; kz0 < nz; kz0 += kMaxGroupVars) {
      chunk(kz0, std::min(kMaxGroupVars, nz - kz0));
      if (int rc = solve_batch_path(v, g0, nb, ncnt, nidx, infob, b2, dn)) return rc;
    }
    return CWBL_OK;
  }
  const TreeDesc *dtrees = S.tdesc.as<TreeDesc>();
  const long long Bs = record_sub_batch(nb);
  if (!crec) HIPCHK(S.wsa.ensure((size_t)(Bs + 1) * 8 * AsmRecord<kTq4KP>::WORDS));
  // a cached batch keeps every sub-batch's records, S.wsa only the current one's
  const size_t rstep = crec ? AsmRecord<kTq4KP>::WORDS : 0;
  int kt;
  for (long long s0 = 0; s0 < nb; s0 += Bs) {
    const int ns = (int)std::min<long long>(Bs, nb - s0);
    int2 *const inf = infob + s0;
    double *const rec = crec ? crec + (size_t)s0 * rstep : S.wsa.as<double>();
    if (!hit) {
      HIPCHK(kt_begin(S.stream, &kt));
      HIPCHK(launch_assemble_record(S.stream, S.kp, dtrees, v.c, restore.sd, g0 + s0, ns,
                                    ncnt + s0 * v.nt, nidx + s0 * v.list_cap, inf, rec));
      HIPCHK(kt_end(S.stream, kt, KT_ASSEMBLE_RECORD, ns));
    }
    if (column_kernel) {
      const int lw = column_levels_per_wave(ns, nz);
      CI.levels_per_wave = lw;
      HIPCHK(kt_begin(S.stream, &kt));
      HIPCHK(launch_solve_tq40_column(S.stream, S.kp, v.c, v.full, g0 + s0, ns, nz, lw, rec, inf));
      HIPCHK(kt_end(S.stream, kt, KT_SOLVE_TQ40_COLUMN, (long long)ns * nz));
      continue;
    }
    for (int kz0 = 0; kz0 < nz; kz0 += kMaxGroupVars) {
      const int n = std::min(kMaxGroupVars, nz - kz0);
      chunk(kz0, n);
      HIPCHK(kt_begin(S.stream, &kt));
      if (n > 1)
        HIPCHK(launch_solve_tq40_multi(S.stream, S.kp, v.c, v.sd, v.tv, g0 + s0, ns, rec, inf));
      else
        HIPCHK(launch_solve_tq40(S.stream, S.kp, v.c, v.sd, g0 + s0, ns, rec, inf));
      HIPCHK(kt_end(S.stream, kt, n > 1 ? KT_SOLVE_TQ40_MULTI : KT_SOLVE_TQ40, (long long)ns * n));
    }
  }
  return CWBL_OK;
}

// After the last batch: the info of the open window, tune_q on the resident slab
// (letkf_driver's Q species post-step, :253-278), the host slab's var back, one
// synchronisation, and the statistics.
int finish_call(VarCall &v, cwbl_stats &st) {
  DevStats *dst = S.stats.as<DevStats>();
  if (v.npts > v.win0) {
    HIPCHK(launch_reduce_info(S.stream, S.info.as<int2>(), (int)(v.npts - v.win0), dst));
    if (int rc = keep_info(v, v.npts)) return rc;
  }
  int ev = v.ev;
  // letkf_tune_q on the variables that ask for it (tune_batch: every batch has had its own)
  for (int i = 0; i < v.nvar && !v.tune_batch; ++i) {
    if (!v.vp[i].tune_q) continue;
    hipEvent_t a, b;
    HIPCHK(event(ev, &a));
    HIPCHK(event(ev + 1, &b));
    HIPCHK(hipEventRecord(a, S.stream));
    SlabDev sdi = v.colshare ? v.full : v.sd;  // (a shared call: the slab, not its column view)
    sdi.var = v.tv.var[i];
    int kt;
    HIPCHK(kt_begin(S.stream, &kt));
    HIPCHK(launch_tune_q(S.stream, sdi, S.k));
    HIPCHK(kt_end(S.stream, kt, KT_TUNE_Q, v.npts * v.nlev));
    ++TI.tune_q_launches;
    HIPCHK(hipEventRecord(b, S.stream));
    v.solve_ev.push_back({ev, ev + 1});
    ev += 2;
  }
  hipEvent_t e_end, e_back;
  HIPCHK(event(ev, &e_end));
  HIPCHK(event(ev + 1, &e_back));
  if (v.host && !v.piped_back && !v.bounce)
    for (int i = 0; i < v.nvar; ++i) {
      HIPCHK(hipMemcpyAsync(v.sl[i].var, v.tv.var[i], v.bvar, hipMemcpyDeviceToHost, S.stream));
      TI.bytes_whole_down += (long long)v.bvar;
    }
  if (v.piped_back) {  // the call returns after the last batch's copy back
    HIPCHK(hipEventRecord(e_back, S.d2h));
    HIPCHK(hipStreamWaitEvent(S.stream, e_back, 0));
  }
  const long long nbat = (long long)v.plan.size();
  if (v.bounce && v.piped_back)  // drain the last batches
    for (long long bj = std::max<long long>(0, nbat - (State::kSlots - 1)); bj < nbat; ++bj)
      if (int rc = bounce_drain(v, bj)) return rc;
  if (v.bounce && !v.piped_back)  // the whole slab back (after tune_q, or a staggered slab)
    if (int rc = bounce_whole(v, false)) return rc;
  HIPCHK(hipEventRecord(e_end, S.stream));
  DevStats ds;
  HIPCHK(hipMemcpyAsync(&ds, S.stats.p, sizeof ds, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  kt_collect();
  prep_collect();

  // (a column-shared call counted its columns: every level of a column has the column's
  // lists, p and quadrature level, so the per-point call's totals are nlev times these)
  const long long lev = v.nlev;
  st.solved = (long long)ds.solved * lev;
  st.nobs_sum = (long long)ds.nobs_sum * lev;
  // (a hit ran none, or only the uncached batches', of the searches that count this: the
  // inputs being equal, the fill's total per level holds)
  st.lz_truncated = (v.reuse != 2 ? (long long)ds.lz_truncated : v.cache->lz_truncated) * lev;
  st.nonconverged = (long long)ds.nonconverged * lev;
  st.sweeps_sum = (long long)ds.sweeps_sum * lev;
  st.max_p = (int)ds.max_p;
  st.max_sweeps = (int)ds.max_sweeps;
  st.ms_prep = elapsed(0, 1);
  for (auto &p : v.search_ev) st.ms_search += elapsed(p.first, p.second);
  for (auto &p : v.solve_ev) st.ms_solve += elapsed(p.first, p.second);
  // copies: x, y, alt (+ var when not piped) before the batches, var back after the last
  // solve; piped transfers overlap the batches and are not counted here
  st.ms_copy = elapsed(1, 2) + (v.host && !v.piped_back ? elapsed(ev - 1, ev) : 0.0f);
  if (v.bounce) st.ms_copy = g_bounce_ms;  // the host threads' bounce copies
  return CWBL_OK;
}

}  // namespace

int set_last_error(int code, const char *msg) {
  g_err = msg;
  return code;
}

}  // namespace cwbl

using namespace cwbl;

extern "C" {

int cwbl_abi_version(void) { return CWBL_ABI_VERSION; }

const char *cwbl_last_error(void) { return g_err.c_str(); }

int cwbl_init(const cwbl_init_params *p) {
  if (!p) return fail(CWBL_ERR_ARG, "cwbl_init: null params");
  if (S.inited) release_all();
  if (p->nmember < 2) return fail(CWBL_ERR_ARG, "nmember must be >= 2 (got %d)", p->nmember);
  const int kp = supported_kp(p->nmember);
  if (kp < 0)
    return fail(CWBL_ERR_UNSUPPORTED, "nmember %d > %d not supported by this build",
                p->nmember, CWBL_MAX_MEMBERS);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(CWBL_ERR_NO_DEVICE, "no HIP device available (the core has no CPU path)");
  int dev = p->device;
  if (dev < 0) HIPCHK(hipGetDevice(&dev));
  if (dev >= ndev) return fail(CWBL_ERR_NO_DEVICE, "device %d >= device count %d", dev, ndev);
  HIPCHK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(CWBL_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950", dev,
                prop.gcnArchName);
  if (p->weight_function != 0 && p->weight_function != 1)
    return fail(CWBL_ERR_ARG, "weight_function must be 0 or 1");
  S.k = p->nmember;
  S.kp = kp;
  S.device = dev;
  S.wf = p->weight_function;
  S.norain = p->norain_value;
  S.q1_mode = p->q1_mode;
  S.ws_bytes = p->workspace_bytes ? p->workspace_bytes : (size_t(2) << 30);
  size_t fr = 0, tot = 0;
  HIPCHK(hipMemGetInfo(&fr, &tot));
  if (p->workspace_bytes) {
    S.handoff_budget = p->workspace_bytes;
  } else {  // 13 GB (98 304 points at k = 128), at most 40% of what is free now
    S.handoff_budget = std::min<size_t>((size_t)13 << 30, fr / 10 * 4);
  }
  // records kept for reuse (CWBL_OPT_RECORD_REUSE): 40 GiB holds a 300 x 300 x 50 slab's 31 GB
  S.reuse_budget = std::min<size_t>((size_t)40 << 30, fr / 10 * 4);
  ++S.gen;
  HIPCHK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&S.sstream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&S.h2d, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&S.d2h, hipStreamNonBlocking));
  {
    std::vector<double2> tab((size_t)4 * kQuadLevels * kQuadStride);  // 15, 23, 31, 63 nodes
    const int rounds[4] = {2, 3, 4, 8};
    for (int r = 0; r < 4; ++r)
      for (int l = 1; l <= kQuadLevels; ++l)
        quad_table(l, &tab[((size_t)r * kQuadLevels + (l - 1)) * kQuadStride],
                   8 * rounds[r] - 1);
    HIPCHK(S.quad.ensure(tab.size() * sizeof(double2)));
    HIPCHK(hipMemcpy(S.quad.p, tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice));
  }
  // path options (cwbl_set_option): every one back to its default
  S.jacobi = false;
  S.tq4 = 1;
  S.tq4_sub = 0;
  S.big_split = true;
  // (C4 per variable, r3: 32 k points 2.42 s, 16 k 2.47, 64 k 2.41, 96 k 2.39, 128 k 2.39)
  S.big_sub = 98304;
  S.binned = true;
  S.pageable_register = true;
  S.bin_div = 0;  // 0: by density (bin_div_for)
  S.index_mode = 0;
  S.index_order = 0;
  S.column_share = 0;
  S.column_levels = 0;
  S.column_factor = false;
  S.column_rows = false;
  S.column_reuse = 0;
  S.factor_reuse = true;
  S.hit_merge = true;
  S.wave_reuse = false;
  S.big_reuse = false;
  S.rows_reuse = false;
  S.host_pipe = false;
  S.ncu = prop.multiProcessorCount;
  std::memset(&P, 0, sizeof P);
  std::memset(&IX, 0, sizeof IX);
  g_index_use.clear();
  g_index_called = false;
  std::memset(&CI, 0, sizeof CI);
  std::memset(&CR, 0, sizeof CR);
  std::memset(&TI, 0, sizeof TI);
  S.lead_div = 0;
  S.serial_search = false;
#ifdef CWBL_DEBUG_KNOBS
  if (const char *e = std::getenv("CWBL_DEBUG_SERIAL")) S.serial_search = std::atoi(e) != 0;
#endif
  S.kp_natural = kp;
  select_kp();
  S.max_batch = 160000;
  S.max_batch_set = false;
  S.info_window = 1LL << 25;
  S.inited = true;
  return CWBL_OK;
}

int cwbl_set_option(int option, long long value) {
  if (!S.inited) return fail(CWBL_ERR_STATE, "cwbl_set_option before cwbl_init");
  auto range = [&](long long lo, long long hi) { return value >= lo && value <= hi; };
  if (option == CWBL_OPT_HIT_MERGE || option == CWBL_OPT_HOST_PIPE ||
      option == CWBL_OPT_COLUMN_FACTOR) {
    // how the cached batches are launched, how a host slab travels, or how a shared call (which
    // touches no cache) solves its levels, not what is cached: the generation stays
    if (!range(0, 1))
      return fail(CWBL_ERR_ARG, "cwbl_set_option: value %lld out of range for option %d", value,
                  option);
    if (option == CWBL_OPT_COLUMN_FACTOR) {
      S.column_factor = value == 1;
      if (!S.column_factor) {  // off holds no memory
        (void)hipStreamSynchronize(S.stream);
        S.wsf.release();
      }
      return CWBL_OK;
    }
    (option == CWBL_OPT_HIT_MERGE ? S.hit_merge : S.host_pipe) = value == 1;
    return CWBL_OK;
  }
  if (option == CWBL_OPT_COLUMN_LEVELS) {
    // how many levels a wavefront of a column or level kernel takes: neither cache keeps
    // anything that depends on it, and a column cache's hit may be split otherwise than its fill
    if (!range(0, 1 << 30))
      return fail(CWBL_ERR_ARG, "cwbl_set_option: value %lld out of range for option %d", value,
                  option);
    S.column_levels = (int)value;
    return CWBL_OK;
  }
  ++S.gen;  // options change the neighbour order and the batch plan: kept records are void
  switch (option) {
    case CWBL_OPT_SOLVER:
      if (!range(0, 1)) break;
      if (value == 1 && S.kp_natural > kMaxWaveKP)
        return fail(CWBL_ERR_UNSUPPORTED, "the Jacobi solver supports k <= %d", kMaxWaveKP);
      S.jacobi = value == 1;
      select_kp();
      return CWBL_OK;
    case CWBL_OPT_SPLIT40:
      if (!range(0, 1)) break;
      S.tq4 = (int)value;
      select_kp();
      return CWBL_OK;
    case CWBL_OPT_SPLIT40_BATCH:
      if (!range(0, 1 << 19)) break;
      S.tq4_sub = value;
      return CWBL_OK;
    case CWBL_OPT_SEARCH:
      if (!range(0, 1)) break;
      S.binned = value == 0;
      return CWBL_OK;
    case CWBL_OPT_BIG_PATH:
      if (!range(0, 1)) break;
      S.big_split = value == 1;
      return CWBL_OK;
    case CWBL_OPT_BIG_BATCH:
      if (!range(64, 1LL << 24)) break;
      S.big_sub = value;
      return CWBL_OK;
    case CWBL_OPT_PAGEABLE:
      if (!range(0, 1)) break;
      S.pageable_register = value == 0;
      return CWBL_OK;
    case CWBL_OPT_BIN_DIV:
      if (!range(0, 8)) break;
      S.bin_div = (int)value;
      return CWBL_OK;
    case CWBL_OPT_LEAD_DIV:
      if (!range(0, 1 << 20)) break;
      S.lead_div = (int)value;
      return CWBL_OK;
    case CWBL_OPT_MAX_BATCH:
      if (value != 0 && !range(256, 1LL << 31)) break;
      S.max_batch = value ? value : 160000;
      S.max_batch_set = value != 0;  // an explicit cap is used as given
      return CWBL_OK;
    case CWBL_OPT_INFO_WINDOW:
      if (value != 0 && !range(256, 1LL << 30)) break;
      S.info_window = value ? value : (1LL << 25);
      return CWBL_OK;
    case CWBL_OPT_INDEX:
      if (!range(0, 1)) break;
      S.index_mode = (int)value;
      return CWBL_OK;
    case CWBL_OPT_INDEX_ORDER:
      if (!range(0, 1)) break;
      S.index_order = (int)value;  // (read under CWBL_OPT_INDEX = 1 only: index_entry)
      return CWBL_OK;
    case CWBL_OPT_COLUMN_SHARE:
      if (!range(0, 2)) break;
      S.column_share = (int)value;
      return CWBL_OK;
    case CWBL_OPT_RECORD_REUSE:
      if (!range(0, 1LL << 24)) break;
      S.reuse_budget = (size_t)value << 20;
      S.cache.release();  // the next fill allocates within the new budget
      return CWBL_OK;
    case CWBL_OPT_FACTOR_REUSE:
      if (!range(0, 1)) break;
      S.factor_reuse = value == 1;  // (the new generation voids a cache of the other form)
      return CWBL_OK;
    case CWBL_OPT_WAVE_REUSE:
      if (!range(0, 1)) break;
      S.wave_reuse = value == 1;
      if (S.cache.form == CacheForm::WaveFactor) S.cache.release();  // off holds no memory
      return CWBL_OK;
    case CWBL_OPT_BIG_REUSE:
      if (!range(0, 1)) break;
      S.big_reuse = value == 1;
      if (S.cache.form == CacheForm::BigFactor) S.cache.release();  // off holds no memory
      return CWBL_OK;
    case CWBL_OPT_ROWS_REUSE:
      if (!range(0, 1)) break;
      S.rows_reuse = value == 1;
      if (S.cache.form == CacheForm::BigFactor) S.cache.release();  // off holds no memory
      return CWBL_OK;
    case CWBL_OPT_COLUMN_REUSE:
      if (!range(0, 1LL << 24)) break;
      S.column_reuse = (size_t)value << 20;
      (void)hipStreamSynchronize(S.stream);
      S.ccache.release();  // 0 holds no memory; the next fill allocates within the new budget
      return CWBL_OK;
    case CWBL_OPT_COLUMN_ROWS:
      // (which classes fill and read the column cache: a new generation, like every option that
      // decides what is cached)
      if (!range(0, 1)) break;
      (void)hipStreamSynchronize(S.stream);
      S.column_rows = value == 1;
      if (!S.column_rows && S.kp == kBigSplitKP) {  // off holds no memory
        S.wsf.release();
        S.ccache.release();
      }
      return CWBL_OK;
    default:
      return fail(CWBL_ERR_ARG, "cwbl_set_option: unknown option %d", option);
  }
  return fail(CWBL_ERR_ARG, "cwbl_set_option: value %lld out of range for option %d", value,
              option);
}

int cwbl_set_stream(void *stream) {
  if (int rc = require_device()) return rc;
  S.caller_stream = static_cast<hipStream_t>(stream);
  return CWBL_OK;
}

int cwbl_set_kernel_timing(int enable) {
  if (int rc = require_device()) return rc;
  S.ktiming = enable != 0;
  for (KTime &t : S.ktime) t = KTime{};
  return CWBL_OK;
}

int cwbl_kernel_times(cwbl_kernel_time *out, int cap, int *n) {
  if (int rc = require_device()) return rc;
  if (!n || cap < 0 || (cap > 0 && !out)) return fail(CWBL_ERR_ARG, "cwbl_kernel_times: bad arguments");
  int m = 0;
  for (int id = 0; id < KT_COUNT; ++id) {
    const KTime &t = S.ktime[id];
    if (t.launches == 0) continue;
    if (m < cap) {
      cwbl_kernel_time &o = out[m];
      std::memset(&o, 0, sizeof o);
      std::snprintf(o.name, sizeof o.name, "%s", kernel_name(id).c_str());
      o.launches = t.launches;
      o.points = t.points;
      o.ms = t.ms;
    }
    ++m;
  }
  *n = m;
  return CWBL_OK;
}

int cwbl_reuse_info(cwbl_reuse_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_reuse_info: null argument");
  *out = R;
  return CWBL_OK;
}

int cwbl_column_info(cwbl_column_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_column_info: null argument");
  *out = CI;
  return CWBL_OK;
}

int cwbl_column_reuse_info(cwbl_column_reuse_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_column_reuse_info: null argument");
  *out = CR;
  return CWBL_OK;
}

int cwbl_transfer_info(cwbl_transfer_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_transfer_info: null argument");
  *out = TI;
  return CWBL_OK;
}

int cwbl_finalize(void) {
  if (S.inited) {
    (void)hipStreamSynchronize(S.stream);
    release_all();
  }
  return CWBL_OK;
}

int cwbl_set_obs(const cwbl_obs_set *o) {
  if (int rc = require_device()) return rc;
  if (!o) return fail(CWBL_ERR_ARG, "null obs set");
  if (o->n_gts < 0 || o->n_radar < 0 || (o->n_gts && !o->gts) || (o->n_radar && !o->radar))
    return fail(CWBL_ERR_ARG, "bad obs set counts/pointers");
  release_obs();
  ++S.gen;  // (the record cache keeps its allocation: only its contents are void)
  const int mem = o->memory;
  if (mem == CWBL_MEM_DEVICE) HIPCHK(order_after_caller());
  const size_t k = (size_t)S.k;
  bool seen_g[CWBL_NUM_GTS_TYPES + 1] = {}, seen_r[CWBL_NUM_RADAR_TYPES + 1] = {};
  for (int e = 0; e < o->n_gts; ++e) {
    const cwbl_gts_obs &g = o->gts[e];
    if (g.type_id < 1 || g.type_id > CWBL_NUM_GTS_TYPES || seen_g[g.type_id])
      return fail(CWBL_ERR_ARG, "gts entry %d: bad or duplicate type_id %d", e, g.type_id);
    if (g.nvar < 1 || g.nvar > CWBL_MAX_NVAR || g.nobs < 0)
      return fail(CWBL_ERR_ARG, "gts type %d: bad nvar/nobs", g.type_id);
    if (g.nobs > 0 && (!g.xyz || !g.obs || !g.error || !g.hdxb || !g.qc))
      return fail(CWBL_ERR_ARG, "gts type %d: null array", g.type_id);
    seen_g[g.type_id] = true;
    S.obs.emplace_back();
    ObsType &t = S.obs.back();
    t.family = 0; t.type_id = g.type_id; t.nvar = g.nvar; t.nobs = g.nobs;
    const size_t n = (size_t)g.nobs, nv = (size_t)g.nvar;
    t.xyz.resize(3 * n);
    if (n) {
      if (mem == CWBL_MEM_DEVICE)
        HIPCHK(hipMemcpyAsync(t.xyz.data(), g.xyz, 3 * n * 4, hipMemcpyDeviceToHost, S.stream));
      else
        std::memcpy(t.xyz.data(), g.xyz, 3 * n * 4);
    }
    HIPCHK(stage(t.obs, g.obs, n * nv * 4, mem));
    HIPCHK(stage(t.error, g.error, n * nv * 4, mem));
    HIPCHK(stage(t.hdxb, g.hdxb, n * nv * k * 4, mem));
    HIPCHK(stage(t.qc, g.qc, n * nv * k * 4, mem));
  }
  for (int e = 0; e < o->n_radar; ++e) {
    const cwbl_radar_obs &r = o->radar[e];
    if (r.type_id < 1 || r.type_id > CWBL_NUM_RADAR_TYPES || seen_r[r.type_id])
      return fail(CWBL_ERR_ARG, "radar entry %d: bad or duplicate type_id %d", e, r.type_id);
    if (r.nobs < 0) return fail(CWBL_ERR_ARG, "radar type %d: bad nobs", r.type_id);
    if (r.nobs > 0 && (!r.xyz || !r.obs || !r.hdxb))
      return fail(CWBL_ERR_ARG, "radar type %d: null array", r.type_id);
    seen_r[r.type_id] = true;
    S.obs.emplace_back();
    ObsType &t = S.obs.back();
    t.family = 1; t.type_id = r.type_id; t.nvar = 1; t.nobs = r.nobs;
    const size_t n = (size_t)r.nobs;
    t.xyz.resize(3 * n);
    if (n) {
      if (mem == CWBL_MEM_DEVICE)
        HIPCHK(hipMemcpyAsync(t.xyz.data(), r.xyz, 3 * n * 4, hipMemcpyDeviceToHost, S.stream));
      else
        std::memcpy(t.xyz.data(), r.xyz, 3 * n * 4);
    }
    HIPCHK(stage(t.obs, r.obs, n * 4, mem));
    HIPCHK(stage(t.hdxb, r.hdxb, n * k * 4, mem));
  }
  HIPCHK(hipStreamSynchronize(S.stream));
  S.have_obs = true;
  return CWBL_OK;
}

// The argument checks of a call's slab and parameters (a group: of its variable 0), before
// any device work.
static int check_slab(const cwbl_var_params *vp, const cwbl_slab *sl) {
  if (!vp || !sl) return fail(CWBL_ERR_ARG, "null argument");
  if (sl->nx < 0 || sl->ny < 0 || sl->nz < 0 || sl->ix_lim < 0 || sl->iy_lim < 0 ||
      sl->ix_lim > sl->nx || sl->iy_lim > sl->ny || sl->ix_lim > sl->alt_nx ||
      sl->iy_lim > sl->alt_ny)
    return fail(CWBL_ERR_ARG, "slab bounds: nx=%d ny=%d ix_lim=%d iy_lim=%d alt=%dx%d",
                sl->nx, sl->ny, sl->ix_lim, sl->iy_lim, sl->alt_nx, sl->alt_ny);
  if (!(vp->multi_infl > 0.0f)) return fail(CWBL_ERR_ARG, "multi_infl must be > 0");
  const long long npts = (long long)sl->ix_lim * sl->iy_lim * sl->nz;
  if (npts >= (1LL << 32))  // the kernels enumerate a slab's points in 32 bits
    return fail(CWBL_ERR_ARG, "slab of %lld points: at most 2^32 - 1 per call", npts);
  return CWBL_OK;
}

// The call is ordered behind the caller's work on a device slab, and the per-call counters
// and spans start empty.
static int begin_call(const cwbl_slab *sl) {
  if (sl->memory == CWBL_MEM_DEVICE) HIPCHK(order_after_caller());
  S.kpend.clear();  // (an earlier call that failed midway leaves nothing to collect)
  S.kev_used = 0;
  g_bounce_ms = 0.0;
  std::memset(&P, 0, sizeof P);
  std::memset(&IX, 0, sizeof IX);
  g_index_use.clear();
  g_index_called = true;
  std::memset(&R, 0, sizeof R);
  std::memset(&CI, 0, sizeof CI);
  std::memset(&CR, 0, sizeof CR);
  std::memset(&TI, 0, sizeof TI);
  g_pspans.clear();
  g_pev_used = 0;
  return CWBL_OK;
}

// CWBL_OPT_HIT_MERGE.  A call that hits has no search for a solve to overlap, so its cached
// batches need not be launched one by one: each launch pays a ramp, a drain tail in which
// every wave slot idles from its last wave's end to the slowest wave's, and the boundary
// with its events (profiles/hit_merge.txt).  The segments of a cached batch are what
// solve_batch_path launches for it: the batch, or its sub-batches under CWBL_OPT_SPLIT40_BATCH.
static long long hit_segments(int nb, long long *Bs_out = nullptr) {
  const long long Bs = record_sub_batch(nb);
  if (Bs_out) *Bs_out = Bs;
  return Bs >= nb ? 1 : (nb + Bs - 1) / Bs;
}

// HitLevelCuts for a call's inflat and k: cuts.t[i] is the smallest trace for which
// solve_tq40_kernel's level loop (dec = 10, 100, ... while dec < trace / m - (k - 1)) ends above
// level n = kRoundCuts[i], i.e. for which 10^n < trace / m - (k - 1) in the kernel's two rounded
// operations.  For m >= 0 neither the quotient nor the difference decreases with the trace (at
// m = 0 the quotient of a zero trace is NaN, which fails the test between the traces that give
// -inf and +inf), so the traces that pass are those from the smallest one on: bisection over
// the doubles in their order.  NaN where not even +inf passes.  False for another m.
static bool hit_level_cuts(float inflat, int k, HitLevelCuts &cuts) {
  const double m = (double)inflat, km1 = (double)(k - 1);
  if (!(m >= 0.0)) return false;
  // the doubles -inf .. +inf as unsigned integers in the same order, and back
  auto key = [](double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return (b >> 63) ? ~b : b | (1ull << 63);
  };
  auto val = [](uint64_t u) {
    const uint64_t b = (u >> 63) ? u & ~(1ull << 63) : ~u;
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
  };
  for (int i = 0; i < 3; ++i) {
    double dec = 10.0;  // (the kernel's products: exact)
    for (int n = 1; n < kRoundCuts[i]; ++n) dec *= 10.0;
    auto above = [&](double t) {
      volatile double q = t / m;  // (two rounded operations, as on the device)
      const double ratio = q - km1;
      return dec < ratio;
    };
    uint64_t lo = key(-HUGE_VAL), hi = key(HUGE_VAL);
    if (!above(val(hi))) {
      cuts.t[i] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    while (lo < hi) {  // above(val(hi)) holds
      const uint64_t mid = lo + (hi - lo) / 2;
      if (above(val(mid))) hi = mid;
      else lo = mid + 1;
    }
    cuts.t[i] = val(hi);
  }
  return true;
}

// Whether the call's cached batches go out merged, and room for their segment tables.
static int plan_hit_merge(VarCall &v, CacheForm form) {
  // (the other factor forms' hits are one launch per batch or sub-batch)
  v.merge = S.hit_merge && form == CacheForm::Tq40Factor && v.reuse == 2 && !v.group &&
            !v.colshare && !v.piped && !v.piped_back && !v.bounce && v.ncached > 0 &&
            hit_level_cuts(v.c.inflat, v.c.k, v.cuts);
  if (!v.merge) return CWBL_OK;
  long long nseg = 0;
  for (long long bi = 0; bi < v.ncached; ++bi) nseg += hit_segments(v.plan[bi].second);
  if (nseg > 65535) {  // (a grid's rows; one launch may have to hold them all)
    v.merge = false;
    return CWBL_OK;
  }
  // grow-only: nothing is allocated from the second hit of a slab on
  HIPCHK(S.hitseg.ensure((size_t)nseg * sizeof(HitSeg)));
  HIPCHK(S.hitseg_pin.ensure((size_t)nseg * sizeof(HitSeg)));
  return CWBL_OK;
}

// The hits of the cached batches [b0, b1), which lie in the open info window, in one launch
// between the events b2 and dn.  Their segments go up ahead of b2, from page-locked memory
// that the call writes once (each launch its own entries), into a table that only grows.
static int solve_hits_merged(VarCall &v, long long b0, long long b1, hipEvent_t b2,
                             hipEvent_t dn) {
  const Cache &C = *v.cache;
  HitSeg *const hseg = S.hitseg_pin.as<HitSeg>() + v.hitseg_used;
  int nseg = 0, maxns = 0;
  long long pts = 0;
  for (long long bi = b0; bi < b1; ++bi) {
    const long long g0 = v.plan[bi].first;
    const int nb = v.plan[bi].second;
    const long long ord = (long long)(C.off[bi] / AsmRecord<kTq4KP>::WORDS);
    long long Bs;
    hit_segments(nb, &Bs);
    for (long long s0 = 0; s0 < nb; s0 += Bs) {
      const int ns = (int)std::min<long long>(Bs, nb - s0);
      hseg[nseg++] = HitSeg{g0 + s0, ord + s0, ns, (int)(g0 + s0 - v.win0)};
      maxns = std::max(maxns, ns);
    }
    pts += nb;
  }
  HitSeg *const dseg = S.hitseg.as<HitSeg>() + v.hitseg_used;
  HIPCHK(hipMemcpyAsync(dseg, hseg, (size_t)nseg * sizeof(HitSeg), hipMemcpyHostToDevice,
                        S.stream));
  v.hitseg_used += (size_t)nseg;
  HIPCHK(hipEventRecord(b2, S.stream));
  if (S.ktiming) S.kpend.push_back({KT_SOLVE_TQ40_FACTOR, b2, dn, pts});
  HIPCHK(launch_solve_tq40_factor_merged(S.stream, S.kp, v.c, v.sd, dseg, nseg, maxns,
                                         C.rec.as<double>(), C.aux.as<double>(),
                                         S.info.as<int2>(), v.cuts));
  HIPCHK(hipEventRecord(dn, S.stream));
  return CWBL_OK;
}

// A call of the cache v.cache: an equal key makes it a candidate; the coordinates decide.  A
// candidate stages its slab first (staged), so its ms_prep holds the staging and the compare.
// The column cache's equal key means the fill's trees were confirmed 2-D under the same obs set,
// options and type parameters, so the slab is staged as a shared call's before the trees are
// planned.  A call that does not hit invalidates the cache: it fills it, if anything does.
static int cache_candidate(VarCall &v, const CacheKey &key, bool &staged) {
  Cache &C = *v.cache;
  if (C.valid && std::memcmp(&key, &C.key, sizeof key) == 0) {
    if (C.per_column) v.colshare = S.column_share;
    if (int rc = stage_slab(v)) return rc;
    staged = true;
    bool same = false;
    if (int rc = cache_coords_match(v, C, same)) return rc;
    if (same) {
      v.reuse = 2;
      v.ncached = (long long)C.off.size();
      v.full_hit = C.off.size() == C.plan.size();
    }
  }
  if (v.reuse != 2) C.valid = false;
  return CWBL_OK;
}

// Behind finish_call: a fill is complete, so the next call may solve from it; and what the call
// reports of its cache (cwbl_reuse_info, cwbl_column_reuse_info; nbat: the call's batches).
static void complete_cache_call(VarCall &v, const cwbl_stats &st, long long nbat) {
  if (v.reuse == 1) {
    Cache &C = *v.cache;
    C.nt = v.nt;
    C.list_cap = v.list_cap;
    // (per level, as finish_call reads it; a shared call is never in the Q1 undefined case: 0)
    C.lz_truncated = st.lz_truncated / std::max(v.nlev, 1);
    C.q1_undefined = st.q1_undefined;
    C.valid = true;
  }
  if (v.colcache) {
    if (v.reuse == 1) CR.columns_filled = v.cache->units;
    if (v.reuse == 2) CR.columns_reused = v.cache->units;
    if (v.reuse == 2) CR.batches_reused = v.ncached;
  }
  R.batches_reused = v.reuse == 2 && !v.colcache ? v.ncached : 0;  // (the record cache's)
  R.batches_assembled = nbat - R.batches_reused;
}

// The list buffers of batch b: the searches alternate between two pairs.
struct ListBufs { int *cnt, *idx; };
static ListBufs list_buffers(long long b) {
  return (b & 1) ? ListBufs{S.nbr_cnt2.as<int>(), S.nbr_idx2.as<int>()}
                 : ListBufs{S.nbr_cnt.as<int>(), S.nbr_idx.as<int>()};
}

// The driver of cwbl_analyze_var and of the group calls of cwbl_analyze_vars (v.vp, v.sl, and
// for a group v.nvar, v.group and the flags of v.tv are the caller's; the arguments are
// checked).  A group call runs with record reuse off: the cache is not read, filled or
// invalidated.
static int analyze_call(VarCall &v, cwbl_stats *stats) {
  const cwbl_var_params *vp = v.vp;
  const cwbl_slab *sl = v.sl;
  if (int rc = begin_call(sl)) return rc;
  const auto t_start = std::chrono::steady_clock::now();
  cwbl_stats st;
  std::memset(&st, 0, sizeof st);
  const long long npts = (long long)sl->ix_lim * sl->iy_lim * sl->nz;
  st.points = v.npts = npts;
  auto finish = [&]() {
    R.bytes_held = (long long)S.cache.bytes();
    CR.bytes_held = (long long)S.ccache.bytes();
    CR.form = form_column_code(S.ccache.form);
    st.ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (stats) *stats = st;
    return CWBL_OK;
  };
  struct Unregister {  // every page-locked-in-place var, on every return path, once no queued
    VarCall &v;        // copy can still touch it
    ~Unregister() {
      if (v.reg.empty()) return;
      (void)hipStreamSynchronize(S.h2d);
      (void)hipStreamSynchronize(S.d2h);
      (void)hipStreamSynchronize(S.stream);
      (void)hipGetLastError();
      for (float *p : v.reg) (void)hipHostUnregister(p);
      v.reg.clear();
    }
  } unreg{v};

  hipEvent_t e0, e1, e2, e_ready;
  HIPCHK(event(0, &e0));
  HIPCHK(hipEventRecord(e0, S.stream));
  // Column sharing (CWBL_OPT_COLUMN_SHARE): a candidate runs with record reuse off, as a group
  // call does; the planned trees confirm it below.  The call's cache: the column cache
  // (CWBL_OPT_COLUMN_REUSE) for a candidate on a path that option serves, the record cache for a
  // single-variable call that is none; no other call reads, fills or invalidates either.
  CI.reason = column_reason(v);
  const bool col_candidate = CI.reason == CWBL_COLUMN_SHARED;
  v.colcache = col_candidate && !v.group && column_reuse_path() && npts > 0;
  const CacheForm form = v.colcache ? column_form() : call_form();
  if (v.colcache)
    v.cache = &S.ccache;
  else if (!v.group && !col_candidate && form != CacheForm::None && S.reuse_budget > 0 && npts > 0)
    v.cache = &S.cache;
  CacheKey key;
  bool staged = false;
  if (v.cache) {
    make_cache_key(key, vp, sl, v.colcache);
    if (int rc = cache_candidate(v, key, staged)) return rc;
  }
  if (v.full_hit) {
    v.nt = v.cache->nt;
    v.list_cap = v.cache->list_cap;
  } else if (int rc = plan_trees(v)) {
    return rc;
  }
  st.ntrees = v.nt;
  if (v.nt == 0 || npts == 0) {  // `if(all(.not. succeed)) cycle` (:66)
    if (col_candidate) CI.reason = CWBL_COLUMN_REASON_NO_TREES;
    HIPCHK(hipStreamSynchronize(S.stream));
    prep_collect();
    return finish();
  }
  for (const TreeDesc &d : v.descs) st.q1_undefined += d.q1_undef ? npts : 0;
  if (v.full_hit) st.q1_undefined = v.cache->q1_undefined;  // (the column cache's: 0)
  // The planned trees decide whether the call is shared per column, and name the Q1 case.  (A
  // candidate with a tree that is not 2-D would mean column_reason and build_family disagree:
  // it runs per point like any other call that is not eligible, with its record reuse off.)
  for (const TreeDesc &d : v.descs) {
    if (CI.reason == CWBL_COLUMN_SHARED && (d.tree_dim != 2 || d.query3d))
      CI.reason = CWBL_COLUMN_REASON_3D;
    if ((CI.reason == CWBL_COLUMN_SHARED || CI.reason == CWBL_COLUMN_REASON_3D) && d.q1_undef)
      CI.reason = CWBL_COLUMN_REASON_Q1;
  }
  v.colshare = CI.reason == CWBL_COLUMN_SHARED ? S.column_share : 0;
  if (!v.colshare && v.colcache) {  // not shared after all: per point, and no column cache
    v.colcache = false;
    v.cache = nullptr;
    v.reuse = 0;
    v.ncached = 0;
  }
  HIPCHK(event(1, &e1));
  HIPCHK(hipEventRecord(e1, S.stream));
  HIPCHK(event(2, &e2));
  if (!staged)
    if (int rc = stage_slab(v)) return rc;
  HIPCHK(hipEventRecord(e2, S.stream));
  if (v.colshare) {  // the batches run over the column view from here on
    v.full = v.sd;
    v.sd.nz = 1;
    v.nlev = sl->nz;
    v.npts = v.ncol = (long long)sl->ix_lim * sl->iy_lim;
    CI.shared = 1;
    CI.columns = v.ncol;
    CI.levels = v.nlev;
  }
  plan_batches(v);
  if (v.reuse == 2 && v.plan != v.cache->plan) {
    // another batch plan under an equal key: the record cache's call fails; the column cache's
    // is a miss.  (A full hit planned no trees yet; the plan follows their list capacity.)
    if (!v.colcache)
      return fail(CWBL_ERR_STATE, "record reuse: the batch plan changed under an equal key");
    v.reuse = 0;
    v.ncached = 0;
    v.cache->valid = false;
    if (v.full_hit) {
      v.full_hit = false;
      if (int rc = plan_trees(v)) return rc;
      st.ntrees = v.nt;
      v.plan.clear();
      plan_batches(v);
    }
  }
  if (int rc = stage_bounce(v)) return rc;
  if (int rc = alloc_call_buffers(v)) return rc;
  if (v.cache && v.reuse != 2)
    if (int rc = begin_cache_fill(v, key, form)) return rc;
  if (int rc = plan_hit_merge(v, form)) return rc;
  if (int rc = restore_info(v, 0)) return rc;
  HIPCHK(event(3, &e_ready));  // inputs staged and the counters cleared
  HIPCHK(hipEventRecord(e_ready, S.stream));
  HIPCHK(hipStreamWaitEvent(S.sstream, e_ready, 0));

  // The searches run on S.sstream into two list buffers, the solves on S.stream: batch b + 1's
  // search (latency-bound, integer / fp32) overlaps batch b's solve (FP64-bound).  Search b
  // waits for the inputs and for the solve of b - 2 (same buffer); solve b waits for search b.
  // A hit under CWBL_OPT_HIT_MERGE solves the cached batches of an info window in one launch
  // (solve_hits_merged): restore_info, b2, the launch, dn, which every batch it covers has as
  // its done event.
  const long long nbat = (long long)v.plan.size();
  long long searched = -1;         // the batch that a merged launch's iteration searched ahead
  hipEvent_t searched_ev = nullptr;  // the end of the search the solve waits for
  for (long long bi = 0; bi < nbat; ++bi) {
    const long long g0 = v.plan[bi].first;
    const int nb = v.plan[bi].second;
    if (g0 + nb - v.win0 > v.info_cap) {  // close the info window; S.stream orders the reuse
      HIPCHK(launch_reduce_info(S.stream, S.info.as<int2>(), (int)(g0 - v.win0),
                                S.stats.as<DevStats>()));
      if (int rc = keep_info(v, g0)) return rc;
      v.win0 = g0;
      if (int rc = restore_info(v, g0)) return rc;
    }
    int2 *const infob = S.info.as<int2>() + (g0 - v.win0);  // this batch's info
    int *const ncnt = list_buffers(bi).cnt, *const nidx = list_buffers(bi).idx;
    const int ev = v.ev;
    hipEvent_t a, b, b2, dn;
    HIPCHK(event(ev, &a));
    HIPCHK(event(ev + 1, &b));
    HIPCHK(event(ev + 2, &b2));
    HIPCHK(event(ev + 3, &dn));
    // a cached batch: its region of the call's cache; on a hit neither lists nor assembly
    const Cache *const C = bi < v.ncached ? v.cache : nullptr;
    double *const crec = C ? C->rec.as<double>() + C->off[bi] : nullptr;
    const bool has_aux = C && form_has_aux(form);
    const size_t aoff = has_aux ? C->off[bi] / C->words() * FactorAux<kTq4KP>::WORDS : 0;
    double *const caux = has_aux ? C->aux.as<double>() + aoff : nullptr;
    const bool hit = crec && v.reuse == 2;
    if (hit && v.merge) {
      // the cached batches of this window: [bi, be)
      long long be = bi + 1;
      while (be < v.ncached && v.plan[be].first + v.plan[be].second - v.win0 <= v.info_cap) ++be;
      // a partial hit: the first batch past the cached ones is searched while they are solved
      if (be == v.ncached && be < nbat) {
        const ListBufs nl = list_buffers(be);
        if (int rc = search_batch(v, be, nl.cnt, nl.idx, a, b)) return rc;
        v.search_ev.push_back({ev, ev + 1});
        searched = be;
        searched_ev = b;
      }
      if (int rc = solve_hits_merged(v, bi, be, b2, dn)) return rc;
      v.solve_ev.push_back({ev + 2, ev + 3});
      for (long long bj = bi; bj < be; ++bj) v.done_ev.push_back(ev + 3);
      v.ev += 4;
      bi = be - 1;
      continue;
    }
    if (!hit) {
      if (bi != searched) {
        if (int rc = search_batch(v, bi, ncnt, nidx, a, b)) return rc;
        searched_ev = b;
      }
      HIPCHK(hipStreamWaitEvent(S.stream, searched_ev, 0));
    }
    if (v.piped)
      if (int rc = upload_batch_var(v, bi)) return rc;
    HIPCHK(hipEventRecord(b2, S.stream));
    if (v.colshare) {
      if (int rc = solve_batch_column(v, g0, nb, ncnt, nidx, infob, b2, dn, crec, hit)) return rc;
    } else if (int rc = solve_batch_path(v, g0, nb, ncnt, nidx, infob, b2, dn, crec,
                                       crec ? form : CacheForm::None, hit, caux)) {
      return rc;
    }
    HIPCHK(hipEventRecord(dn, S.stream));  // this batch's lists are free again
    hipEvent_t back = dn;  // ... and its analysis final, unless tune_q follows
    if (v.tune_batch) {    // timed from dn to an event of its own, which the copy back waits for
      if (int rc = tune_batch_var(v, g0, nb)) return rc;
      HIPCHK(event(ev + 4, &back));
      HIPCHK(hipEventRecord(back, S.stream));
      v.solve_ev.push_back({ev + 3, ev + 4});
    }
    if (v.piped_back)
      if (int rc = return_batch_var(v, bi, back)) return rc;
    if (v.bounce && v.piped) {  // host side while the GPU works: next batch in, bi - 2 out
      if (bi + 1 < nbat)
        if (int rc = bounce_fill(v, bi + 1)) return rc;
      if (v.piped_back && bi >= State::kSlots - 1)
        if (int rc = bounce_drain(v, bi - (State::kSlots - 1))) return rc;
    }
    if (!hit && bi != searched) v.search_ev.push_back({ev, ev + 1});
    v.solve_ev.push_back({ev + 2, ev + 3});
    v.done_ev.push_back(ev + 3);
    v.ev += v.tune_batch ? 5 : 4;
  }
  if (int rc = finish_call(v, st)) return rc;
  complete_cache_call(v, st, nbat);
  return finish();
}

int cwbl_analyze_var(const cwbl_var_params *vp, const cwbl_slab *sl, cwbl_stats *stats) {
  if (int rc = require_device()) return rc;
  if (!S.have_obs) return fail(CWBL_ERR_STATE, "cwbl_set_obs has not been called");
  if (int rc = check_slab(vp, sl)) return rc;
  VarCall v;
  v.vp = vp;
  v.sl = sl;
  return analyze_call(v, stats);
}

// ---- cwbl_analyze_vars -----------------------------------------------------------------------
// The group rule (include/cwb_letkf_core.h), before any device work.
static int check_group(int nvar, const cwbl_var_params *vp, const cwbl_slab *sl) {
  if (nvar < 1 || nvar > CWBL_MAX_GROUP_VARS)
    return fail(CWBL_ERR_ARG, "cwbl_analyze_vars: nvar = %d, must be 1..%d", nvar,
                CWBL_MAX_GROUP_VARS);
  if (int rc = check_slab(vp, sl)) return rc;
  const cwbl_slab &s0 = sl[0];
  const size_t bvar = (size_t)s0.nx * s0.ny * s0.nz * (size_t)S.k * sizeof(float);
  for (int i = 1; i < nvar; ++i) {
    const cwbl_slab &s = sl[i];
    const struct { const char *name; bool same; } f[] = {
        {"nx", s.nx == s0.nx}, {"ny", s.ny == s0.ny}, {"nz", s.nz == s0.nz},
        {"alt_nx", s.alt_nx == s0.alt_nx}, {"alt_ny", s.alt_ny == s0.alt_ny},
        {"ix_lim", s.ix_lim == s0.ix_lim}, {"iy_lim", s.iy_lim == s0.iy_lim},
        {"memory", s.memory == s0.memory}, {"x (pointer)", s.x == s0.x},
        {"y (pointer)", s.y == s0.y}, {"alt (pointer)", s.alt == s0.alt},
        {"multi_infl", std::memcmp(&vp[i].multi_infl, &vp[0].multi_infl, sizeof(float)) == 0},
        {"gts", std::memcmp(vp[i].gts, vp[0].gts, sizeof vp[0].gts) == 0},
        {"radar", std::memcmp(vp[i].radar, vp[0].radar, sizeof vp[0].radar) == 0}};
    for (const auto &e : f)
      if (!e.same)
        return fail(CWBL_ERR_ARG, "cwbl_analyze_vars: variable %d differs from variable 0 in %s",
                    i, e.name);
  }
  for (int i = 0; i < nvar; ++i)
    for (int j = i + 1; j < nvar && bvar > 0; ++j) {
      const uintptr_t a = (uintptr_t)sl[i].var, b = (uintptr_t)sl[j].var;
      if (a < b + bvar && b < a + bvar)
        return fail(CWBL_ERR_ARG, "cwbl_analyze_vars: the var arrays of variables %d and %d overlap",
                    i, j);
    }
  return CWBL_OK;
}

int cwbl_analyze_vars(int nvar, const cwbl_var_params *vp, const cwbl_slab *slabs,
                      cwbl_stats *stats) {
  if (int rc = require_device()) return rc;
  if (!S.have_obs) return fail(CWBL_ERR_STATE, "cwbl_set_obs has not been called");
  if (int rc = check_group(nvar, vp, slabs)) return rc;
  if (record_path() || ((wave_path() || (handoff_path() && !S.jacobi)) && nvar > 1)) {
    // the fused paths: per search batch (and record sub-batch) one search, one assembly and one
    // solve_tq40_multi_kernel, or one solve_tq_multi_kernel, or one hand-off kernel pair
    // (solve_tq_rows_multi_kernel / solve_tq_big_multi_kernel, solve_tqb_tail_multi_kernel),
    // over all variables
    VarCall v;
    v.vp = vp;
    v.sl = slabs;
    v.nvar = nvar;
    v.group = true;
    v.tv.nvar = nvar;
    for (int i = 0; i < nvar; ++i) {
      v.tv.use_rtpp[i] = vp[i].use_rtpp;
      v.tv.use_rtps[i] = vp[i].use_rtps;
      v.tv.rtpp_alpha[i] = vp[i].rtpp_alpha;
      v.tv.rtps_alpha[i] = vp[i].rtps_alpha;
    }
    return analyze_call(v, stats);
  }
  // every other path (CWBL_OPT_SOLVER = 1, k > 64 under CWBL_OPT_BIG_PATH = 0) and a group of
  // one outside the record path: the variables one after another through cwbl_analyze_var; the
  // counters are the first variable's (they do not depend on the variable), the times summed
  const auto t_start = std::chrono::steady_clock::now();
  cwbl_stats st;
  std::memset(&st, 0, sizeof st);
  for (int i = 0; i < nvar; ++i) {
    cwbl_stats si;
    if (int rc = cwbl_analyze_var(&vp[i], &slabs[i], &si)) return rc;
    if (i == 0) {
      st = si;
    } else {
      st.ms_prep += si.ms_prep;
      st.ms_search += si.ms_search;
      st.ms_solve += si.ms_solve;
      st.ms_copy += si.ms_copy;
    }
  }
  st.ms_total =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  if (stats) *stats = st;
  return CWBL_OK;
}

int cwbl_solve_batch(int npts, const long long *col_off, const float *yo, const float *yb,
                     const float *xb, float inflat, int use_rtpp, float rtpp_alpha,
                     int use_rtps, float rtps_alpha, float *xa, double *evals, int memory) {
  if (int rc = require_device()) return rc;
  if (npts < 0 || (npts > 0 && (!col_off || !xb || !xa)))
    return fail(CWBL_ERR_ARG, "cwbl_solve_batch: bad arguments");
  if (npts == 0) return CWBL_OK;
  const size_t k = (size_t)S.k;
  std::vector<long long> hoff;
  const long long *doff = col_off;
  long long ncol;
  if (memory == CWBL_MEM_DEVICE) {
    HIPCHK(order_after_caller());
    HIPCHK(hipMemcpyAsync(&ncol, col_off + npts, 8, hipMemcpyDeviceToHost, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
  } else {
    ncol = col_off[npts];
    for (int i = 0; i < npts; ++i)
      if (col_off[i + 1] < col_off[i]) return fail(CWBL_ERR_ARG, "col_off not monotone");
  }
  if (ncol > 0 && (!yo || !yb)) return fail(CWBL_ERR_ARG, "cwbl_solve_batch: null yo/yb");
  const float *dyo = yo, *dyb = yb, *dxb = xb;
  float *dxa = xa;
  double *dev = evals;
  if (memory != CWBL_MEM_DEVICE) {
    HIPCHK(stage(S.bcol, col_off, (size_t)(npts + 1) * 8, memory));
    HIPCHK(stage(S.byo, yo, (size_t)ncol * 4, memory));
    HIPCHK(stage(S.byb, yb, (size_t)ncol * k * 4, memory));
    HIPCHK(stage(S.bxb, xb, (size_t)npts * k * 4, memory));
    HIPCHK(S.bxa.ensure((size_t)npts * k * 4));
    if (evals) HIPCHK(S.bev.ensure((size_t)npts * k * 8));
    doff = S.bcol.as<long long>(); dyo = S.byo.as<float>(); dyb = S.byb.as<float>();
    dxb = S.bxb.as<float>(); dxa = S.bxa.as<float>(); dev = evals ? S.bev.as<double>() : nullptr;
  }
  HIPCHK(S.info.ensure((size_t)npts * sizeof(int2)));
  SolveConsts c = solve_consts(inflat, use_rtpp, rtpp_alpha, use_rtps, rtps_alpha);
  // Eigenvalues (dsyevd's ascending eval, module_eigen.f90:48-56): from the tridiagonal T the
  // tq kernels form, by bisection (launch_tridiag_eigvals), at every k; CWBL_OPT_SOLVER = 1
  // (k <= 64) takes them from the Jacobi eigensolver instead.
  const bool jacobi = S.jacobi && S.kp <= kMaxWaveKP;
  double *tri = nullptr;
  if (dev && !jacobi) {
    HIPCHK(S.btri.ensure((size_t)npts * 2 * S.kp * sizeof(double)));
    tri = S.btri.as<double>();
  }
  if (S.kp > kMaxWaveKP)
    HIPCHK(launch_solve_tq_big(S.stream, S.kp, true, nullptr, c, SlabDev{}, 0, npts, nullptr,
                               nullptr, doff, dyo, dyb, dxb, dxa, S.info.as<int2>(), tri));
  else if (jacobi)
    HIPCHK(launch_solve_assembled(S.stream, S.kp, c, npts, doff, dyo, dyb, dxb, dxa, dev,
                                  S.info.as<int2>()));
  else
    HIPCHK(launch_solve_tq(S.stream, S.kp, true, nullptr, c, SlabDev{}, 0, npts, nullptr,
                           nullptr, doff, dyo, dyb, dxb, dxa, S.info.as<int2>(), tri));
  if (tri) HIPCHK(launch_tridiag_eigvals(S.stream, S.kp, S.k, npts, tri, dev));
  if (memory != CWBL_MEM_DEVICE) {
    HIPCHK(hipMemcpyAsync(xa, dxa, (size_t)npts * k * 4, hipMemcpyDeviceToHost, S.stream));
    if (evals)
      HIPCHK(hipMemcpyAsync(evals, dev, (size_t)npts * k * 8, hipMemcpyDeviceToHost, S.stream));
  }
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_pack_columns(const float *global, int nx, int ny, int nz, int px, int py,
                      float *send) {
  if (int rc = require_device()) return rc;
  if (nx < 0 || ny < 0 || nz < 0 || px < 1 || py < 1 || px > kMaxRankDim || py > kMaxRankDim ||
      (((long long)nx * ny * nz) > 0 && (!global || !send)))
    return fail(CWBL_ERR_ARG, "cwbl_pack_columns: bad arguments");
  Decomp d;
  make_decomp(d, nx, ny, nz, px, py);
  HIPCHK(order_after_caller());
  HIPCHK(launch_pack_columns(S.stream, global, d, send));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_unpack_columns(const float *recv, int nx, int ny, int nz, int px, int py,
                        float *global) {
  if (int rc = require_device()) return rc;
  if (nx < 0 || ny < 0 || nz < 0 || px < 1 || py < 1 || px > kMaxRankDim || py > kMaxRankDim ||
      (((long long)nx * ny * nz) > 0 && (!global || !recv)))
    return fail(CWBL_ERR_ARG, "cwbl_unpack_columns: bad arguments");
  Decomp d;
  make_decomp(d, nx, ny, nz, px, py);
  HIPCHK(order_after_caller());
  HIPCHK(launch_unpack_columns(S.stream, recv, d, global));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_pack_members(const float *global, long long gstride, int nm, int nx, int ny, int nz,
                      int px, int py, float *send, long long sstride) {
  if (int rc = require_device()) return rc;
  const long long n = (long long)nx * ny * nz;
  if (nx < 0 || ny < 0 || nz < 0 || px < 1 || py < 1 || px > kMaxRankDim || py > kMaxRankDim ||
      nm < 0 || nm > 65535 || (nm > 1 && (gstride < n || sstride < n)) ||
      (n > 0 && nm > 0 && (!global || !send)))
    return fail(CWBL_ERR_ARG, "cwbl_pack_members: bad arguments");
  Decomp d;
  make_decomp(d, nx, ny, nz, px, py);
  HIPCHK(order_after_caller());
  HIPCHK(launch_transpose_columns(S.stream, false, global, gstride, nm, d, send, sstride));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_unpack_members(const float *recv, long long rstride, int nm, int nx, int ny, int nz,
                        int px, int py, float *global, long long gstride) {
  if (int rc = require_device()) return rc;
  const long long n = (long long)nx * ny * nz;
  if (nx < 0 || ny < 0 || nz < 0 || px < 1 || py < 1 || px > kMaxRankDim || py > kMaxRankDim ||
      nm < 0 || nm > 65535 || (nm > 1 && (gstride < n || rstride < n)) ||
      (n > 0 && nm > 0 && (!global || !recv)))
    return fail(CWBL_ERR_ARG, "cwbl_unpack_members: bad arguments");
  Decomp d;
  make_decomp(d, nx, ny, nz, px, py);
  HIPCHK(order_after_caller());
  HIPCHK(launch_transpose_columns(S.stream, true, recv, rstride, nm, d, global, gstride));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_vcoord_mean(const float *ph, long long n2d, int nz_ph, int k, int stagger, float g,
                     float *alt) {
  if (int rc = require_device()) return rc;
  if (n2d < 0 || k < 1 || (stagger != 0 && stagger != 1) || nz_ph < (stagger == 0 ? 2 : 1) ||
      (n2d > 0 && (!ph || !alt)))
    return fail(CWBL_ERR_ARG, "cwbl_vcoord_mean: bad arguments");
  // alpha = 1.0/(g*nmember) in default real (module_mpi_util.f90:496)
  const float gk = g * (float)k;
  const float alpha = 1.0f / gk;
  HIPCHK(order_after_caller());
  HIPCHK(launch_vcoord_mean(S.stream, ph, n2d, nz_ph, k, stagger, alpha, alt));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_member_sum(const float *fields, long long n, int nm, float *out) {
  if (int rc = require_device()) return rc;
  if (n < 0 || nm < 1 || (n > 0 && (!fields || !out)))
    return fail(CWBL_ERR_ARG, "cwbl_member_sum: bad arguments");
  HIPCHK(order_after_caller());
  HIPCHK(launch_member_sum(S.stream, fields, n, nm, out));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_scale(float *x, long long n, float alpha) {
  if (int rc = require_device()) return rc;
  if (n < 0 || (n > 0 && !x)) return fail(CWBL_ERR_ARG, "cwbl_scale: bad arguments");
  HIPCHK(order_after_caller());
  HIPCHK(launch_scale(S.stream, x, n, alpha));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_search(int nobs, const float *obs_xyz, float hclr, float vclr, int max_lz_pts,
                int nq, const float *q_xyz, int *nfound, int *idx, float *r2, int memory) {
  if (int rc = require_device()) return rc;
  if (nobs < 0 || nq < 0 || max_lz_pts < 1 || !(hclr > 0.0f))
    return fail(CWBL_ERR_ARG, "cwbl_search: bad arguments");
  if (memory == CWBL_MEM_DEVICE)
    return fail(CWBL_ERR_UNSUPPORTED, "cwbl_search takes host arrays");
  const float hinv = 1.0f / (hclr * 1e3f);
  const float vinv = vclr > 0.0f ? 1.0f / (vclr * 1e3f) : -1.0f;
  const bool dim3 = vinv > 0.0f;
  std::vector<float> nx(3 * (size_t)nobs);
  for (int j = 0; j < nobs; ++j) {
    nx[3 * j] = obs_xyz[3 * j] * hinv;
    nx[3 * j + 1] = obs_xyz[3 * j + 1] * hinv;
    nx[3 * j + 2] = dim3 ? obs_xyz[3 * j + 2] * vinv : -1.0f;
  }
  TreeBufs tb;
  build_kdtree(nx.data(), nobs, dim3 ? 3 : 2, tb.host);
  tb.depth = tree_depth(tb.host);
  if (tb.depth >= kSearchStackDepth)
    return fail(CWBL_ERR_UNSUPPORTED, "k-d tree too deep");
  const HostTree &h = tb.host;
  HIPCHK(tb.nodes.ensure(std::max<size_t>(h.nodes.size(), 1) * sizeof(TreeNode)));
  HIPCHK(tb.rdata.ensure(h.rdata.size() * sizeof(float)));
  HIPCHK(tb.ind.ensure(h.ind.size() * sizeof(int) + 4));
  if (!h.nodes.empty())
    HIPCHK(hipMemcpyAsync(tb.nodes.p, h.nodes.data(), h.nodes.size() * sizeof(TreeNode),
                          hipMemcpyHostToDevice, S.stream));
  HIPCHK(hipMemcpyAsync(tb.rdata.p, h.rdata.data(), h.rdata.size() * sizeof(float),
                        hipMemcpyHostToDevice, S.stream));
  if (nobs)
    HIPCHK(hipMemcpyAsync(tb.ind.p, h.ind.data(), h.ind.size() * sizeof(int),
                          hipMemcpyHostToDevice, S.stream));
  TreeDesc d{};
  d.nodes = tb.nodes.as<TreeNode>();
  d.rdata = tb.rdata.as<float4>();
  d.ind = tb.ind.as<int>();
  d.hclr_inv = hinv;
  d.vclr_inv = vinv;
  d.tree_dim = dim3 ? 3 : 2;
  d.query3d = dim3 ? 1 : 0;
  d.nvar = 1;
  d.max_lz = nobs > 0 ? max_lz_pts : 0;
  d.list_off = 0;
  DevBuf dd;
  HIPCHK(dd.ensure(sizeof d));
  HIPCHK(hipMemcpyAsync(dd.p, &d, sizeof d, hipMemcpyHostToDevice, S.stream));
  HIPCHK(stage(S.qxyz, q_xyz, (size_t)nq * 12, CWBL_MEM_HOST));
  HIPCHK(S.qnf.ensure((size_t)nq * 4));
  HIPCHK(S.qidx.ensure((size_t)nq * max_lz_pts * 4));
  HIPCHK(S.qr2.ensure((size_t)nq * max_lz_pts * 4));
  HIPCHK(launch_search_single(S.stream, dd.as<TreeDesc>(), tb.depth, search_r2(), nq,
                              S.qxyz.as<float>(),
                              max_lz_pts, S.qnf.as<int>(), S.qidx.as<int>(), S.qr2.as<float>()));
  HIPCHK(hipMemcpyAsync(nfound, S.qnf.p, (size_t)nq * 4, hipMemcpyDeviceToHost, S.stream));
  HIPCHK(hipMemcpyAsync(idx, S.qidx.p, (size_t)nq * max_lz_pts * 4, hipMemcpyDeviceToHost,
                        S.stream));
  HIPCHK(hipMemcpyAsync(r2, S.qr2.p, (size_t)nq * max_lz_pts * 4, hipMemcpyDeviceToHost,
                        S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  dd.release();
  tb.nodes.release(); tb.rdata.release(); tb.ind.release();
  return CWBL_OK;
}

int cwbl_bin_index(int nobs, const float *obs_xyz, float hclr, float vclr, int div,
                   cwbl_bin_grid *grid, long long start_cap, int *start, int *order,
                   int memory) {
  if (int rc = require_device()) return rc;
  if (nobs < 0 || !(hclr > 0.0f) || div < 0 || div > 8 || !grid || (nobs > 0 && !obs_xyz) ||
      (memory != CWBL_MEM_HOST && memory != CWBL_MEM_DEVICE) ||
      (start && nobs > 0 && !order))
    return fail(CWBL_ERR_ARG, "cwbl_bin_index: bad arguments");
  const float hinv = 1.0f / (hclr * 1e3f);
  const float vinv = vclr > 0.0f ? 1.0f / (vclr * 1e3f) : -1.0f;
  const int tdim = vinv > 0.0f ? 3 : 2;
  if (memory == CWBL_MEM_DEVICE) HIPCHK(order_after_caller());
  HostBins bins;
  int div_used = div > 0 ? div : 2;
  DevBuf dxyz, ncoord, bstart;
  struct Free {
    DevBuf &a, &b, &c;
    ~Free() { a.release(); b.release(); c.release(); }
  } fr{dxyz, ncoord, bstart};
  const int *svals = nullptr;
  auto out_grid = [&]() {
    grid->x0 = bins.x0; grid->y0 = bins.y0; grid->z0 = bins.z0; grid->binv = bins.binv;
    grid->nbx = bins.nbx; grid->nby = bins.nby; grid->nbz = bins.nbz; grid->div = div_used;
  };
  const auto d2 = memory == CWBL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (nobs == 0) {  // the grid of no point: one cell
    const float z[3] = {0.0f, 0.0f, 0.0f};
    bin_grid(z, z, tdim, std::sqrt(search_r2()), div_used, bins);
    out_grid();
    if (!start) return CWBL_OK;
    if (start_cap < 2) return fail(CWBL_ERR_ARG, "cwbl_bin_index: start holds %lld < 2", start_cap);
    HIPCHK(bstart.ensure(2 * sizeof(int)));
    HIPCHK(hipMemsetAsync(bstart.p, 0, 2 * sizeof(int), S.stream));
    HIPCHK(hipMemcpyAsync(start, bstart.p, 2 * sizeof(int), d2, S.stream));
    HIPCHK(hipStreamSynchronize(S.stream));
    return CWBL_OK;
  }
  const float *dx = obs_xyz;
  if (memory != CWBL_MEM_DEVICE) {
    HIPCHK(stage(dxyz, obs_xyz, (size_t)nobs * 12, CWBL_MEM_HOST));
    dx = dxyz.as<float>();
  }
  IndexBounds bounds{};
  if (int rc = device_bins(S.stream, dx, nobs, tdim, hinv, vinv, div, false, bounds, ncoord, bins,
                           div_used, true, nullptr, bstart))
    return rc;
  out_grid();
  if (!start) return CWBL_OK;
  const long long ncell = (long long)bins.nbx * bins.nby * bins.nbz;
  if (start_cap < ncell + 1)
    return fail(CWBL_ERR_ARG, "cwbl_bin_index: start holds %lld < %lld entries", start_cap,
                ncell + 1);
  if (int rc = device_bins(S.stream, dx, nobs, tdim, hinv, vinv, div, true, bounds, ncoord, bins,
                           div_used, false, nullptr, bstart, nullptr, &svals))
    return rc;
  HIPCHK(hipMemcpyAsync(start, bstart.p, (size_t)(ncell + 1) * sizeof(int), d2, S.stream));
  HIPCHK(hipMemcpyAsync(order, svals, (size_t)nobs * sizeof(int), d2, S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

int cwbl_prep_info(cwbl_prep_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_prep_info: null argument");
  *out = P;
  return CWBL_OK;
}

int cwbl_index_info(cwbl_index_info_t *out) {
  if (int rc = require_device()) return rc;
  if (!out) return fail(CWBL_ERR_ARG, "cwbl_index_info: null argument");
  *out = IX;
  return CWBL_OK;
}

int cwbl_index_slots(int family, int type_id, int cap, int *slot_obs, int *n) {
  if (int rc = require_device()) return rc;
  if (!n || cap < 0 || (cap > 0 && !slot_obs))
    return fail(CWBL_ERR_ARG, "cwbl_index_slots: bad arguments");
  if (!g_index_called) return fail(CWBL_ERR_STATE, "cwbl_index_slots before cwbl_analyze_var");
  const TreeBufs *tb = nullptr;
  for (const IndexUse &u : g_index_use)
    if (u.family == family && u.type_id == type_id) tb = u.tb;
  if (!tb)
    return fail(CWBL_ERR_ARG, "cwbl_index_slots: the last call used no obs type %d of family %d",
                type_id, family);
  *n = tb->n;
  const int m = std::min(cap, tb->n);
  if (m <= 0) return CWBL_OK;
  if (tb->mode == 1 && !tb->cell_order) {  // a slot is the obs index
    for (int i = 0; i < m; ++i) slot_obs[i] = i;
    return CWBL_OK;
  }
  const DevBuf &src = tb->mode == 0 ? tb->ind : tb->order;
  HIPCHK(hipMemcpyAsync(slot_obs, src.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost,
                        S.stream));
  HIPCHK(hipStreamSynchronize(S.stream));
  return CWBL_OK;
}

}  // extern "C"
