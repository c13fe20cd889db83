// cwbl_index.hip — the uniform search bins built on the device (CWBL_OPT_INDEX = 1,
// cwbl_bin_index), straight from an obs type's xyz(3,n):
//
//   index_normalize_kernel      xyz -> normalised (x, y, z, 0) in obs order (the fp32 products of
//                               build_family) + per-block partial bounds: per coordinate over
//                               its finite values (build_bins) and over the points whose
//                               coordinates are all finite (the density rule of bin_div_for)
//   (host)                      the grid from the bounds: bin_grid, shared with build_bins
//   index_cells_kernel          cell id per obs with build_bins' fp32 cell arithmetic
//   index_radix_hist/scatter    stable LSD radix sort of (cell id, obs index), 8 bits a pass:
//                               the order inside a cell is ascending obs index, whatever the
//                               cell's length (every obs in one cell included)
//   index_starts_kernel         bstart[c] = first sorted position with cell id >= c
//   index_fill_kernel           bxyz[p] = (x, y, z, obs index as int bits) + the kBinPad tail
//
// and, for columns numbered in the bins' cell order (CWBL_OPT_INDEX_ORDER = 1):
//
//   index_fill_pos_kernel       index_fill_kernel with the sorted position p itself as payload
//   index_rank_kernel           rank[order[p]] = p: the inverse of the sorted obs indices
//   index_compose_kernel        ind2[i] = rank[ind[i]]: a k-d tree's slots as sorted positions
//
// Nothing here depends on the order in which blocks or atomics complete: integer atomics only
// count (the LDS digit histograms), positions come from scans and in-wave ranks.
#include "cwbl_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

namespace cwbl {

namespace {

constexpr float kFltMax = 3.402823466e38f;
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= kFltMax; }  // NaN: false

// ---------------------------------------------------------------------------------------
// normalise + bounds
// ---------------------------------------------------------------------------------------
constexpr int kBoundThreads = 256;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// part[block][12]: lo[3], hi[3] per coordinate over its finite values, then lo[3], hi[3] over
// the points whose `dim` coordinates are all finite; +inf / -inf where nothing was seen
__global__ void __launch_bounds__(kBoundThreads)
index_normalize_kernel(const float *__restrict__ xyz, int n, int dim, float hinv, float vinv,
                       float4 *__restrict__ ncoord, float *__restrict__ part) {
  __shared__ float red[kBoundThreads / 64][kIndexBoundWords];
  float lo[3], hi[3], alo[3], ahi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = alo[c] = INFINITY;
    hi[c] = ahi[c] = -INFINITY;
  }
  for (long long i = (long long)blockIdx.x * kBoundThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kBoundThreads) {
    float v[3];
    v[0] = xyz[3 * i + 0] * hinv;
    v[1] = xyz[3 * i + 1] * hinv;
    v[2] = dim == 3 ? xyz[3 * i + 2] * vinv : 0.0f;  // a 2-D tree's rdata keeps z = 0
    ncoord[i] = make_float4(v[0], v[1], v[2], 0.0f);
    const bool all = finite_f(v[0]) && finite_f(v[1]) && (dim < 3 || finite_f(v[2]));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (finite_f(v[c])) {
        lo[c] = fminf(lo[c], v[c]);
        hi[c] = fmaxf(hi[c], v[c]);
      }
      if (all && c < dim) {
        alo[c] = fminf(alo[c], v[c]);
        ahi[c] = fmaxf(ahi[c], v[c]);
      }
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = wave_min(lo[c]), b = wave_max(hi[c]);
    const float d = wave_min(alo[c]), e = wave_max(ahi[c]);
    if (lane == 0) {
      red[wave][c] = a;
      red[wave][3 + c] = b;
      red[wave][6 + c] = d;
      red[wave][9 + c] = e;
    }
  }
  __syncthreads();
  if (threadIdx.x < kIndexBoundWords) {
    const int j = threadIdx.x;
    const bool is_min = j < 3 || (j >= 6 && j < 9);
    float r = red[0][j];
    for (int w = 1; w < kBoundThreads / 64; ++w)
      r = is_min ? fminf(r, red[w][j]) : fmaxf(r, red[w][j]);
    part[(size_t)blockIdx.x * kIndexBoundWords + j] = r;
  }
}

// ---------------------------------------------------------------------------------------
// cell ids: build_bins' arithmetic in fp32 (a point with a non-finite coordinate: cell 0)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int cell_of(float v, float b0, float binv, int nb) {
  const float f = (v - b0) * binv;
  if (!finite_f(f)) return 0;
  return (int)fminf(fmaxf(floorf(f), 0.0f), (float)(nb - 1));
}

__global__ void __launch_bounds__(256)
index_cells_kernel(const float4 *__restrict__ ncoord, int n, int dim, IndexGrid g,
                   int *__restrict__ keys, int *__restrict__ vals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 d = ncoord[i];
  const bool fin = finite_f(d.x) && finite_f(d.y) && (dim < 3 || finite_f(d.z));
  const int cz = dim == 3 ? cell_of(d.z, g.z0, g.binv, g.nbz) : 0;
  const int cid =
      fin ? cell_of(d.x, g.x0, g.binv, g.nbx) + g.nbx * (cell_of(d.y, g.y0, g.binv, g.nby) + g.nby * cz)
          : 0;
  keys[i] = cid;
  vals[i] = (int)i;
}

// ---------------------------------------------------------------------------------------
// stable LSD radix sort, 8 bits a pass: one wavefront per block of kSortChunk elements
// ---------------------------------------------------------------------------------------
constexpr int kSortRounds = 16;
constexpr int kSortChunk = 64 * kSortRounds;

// hist[d * nblk + b]: elements of block b with digit d (digit-major: its exclusive scan is the
// first output position of (digit, block))
__global__ void __launch_bounds__(64)
index_radix_hist_kernel(const int *__restrict__ kin, int n, int shift, int nblk,
                        int *__restrict__ hist) {
  __shared__ int h[256];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int d = lane; d < 256; d += 64) h[d] = 0;
  __syncthreads();
  for (int r = 0; r < kSortRounds; ++r) {
    const long long i = (long long)b * kSortChunk + r * 64 + lane;
    if (i < n) atomicAdd(&h[(kin[i] >> shift) & 255], 1);
  }
  __syncthreads();
  for (int d = lane; d < 256; d += 64) hist[(size_t)d * nblk + b] = h[d];
}

// in-place exclusive scan of a[0..m) by one block: per-thread segments, a block scan of the
// segment sums, then the segments again
__global__ void __launch_bounds__(1024) index_scan_kernel(int *__restrict__ a, int m) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (m + 1023) / 1024;
  const int b = (int)min((long long)t * per, (long long)m), e = min(b + per, m);
  int s = 0;
  for (int i = b; i < e; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = t ? part[t - 1] : 0;
  for (int i = b; i < e; ++i) {
    const int v = a[i];
    a[i] = base;
    base += v;
  }
}

// Round r of block b takes 64 consecutive elements; an element's position is its (digit,
// block) base plus the elements of the same digit before it in the block: those of earlier
// rounds (base[] is advanced per round) and the lower lanes of this round (the 64-bit ballots).
__global__ void __launch_bounds__(64)
index_radix_scatter_kernel(const int *__restrict__ kin, const int *__restrict__ vin, int n,
                           int shift, int nblk, const int *__restrict__ hist,
                           int *__restrict__ kout, int *__restrict__ vout) {
  __shared__ int base[256];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int d = lane; d < 256; d += 64) base[d] = hist[(size_t)d * nblk + b];
  __syncthreads();
  for (int r = 0; r < kSortRounds; ++r) {
    const long long i = (long long)b * kSortChunk + r * 64 + lane;
    const bool valid = i < n;
    const int key = valid ? kin[i] : 0, val = valid ? vin[i] : 0;
    const int d = (key >> shift) & 255;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1;
      const unsigned long long m = __ballot(one);
      peers &= one ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const int npeer = __popcll(peers);
    const int pos = valid ? base[d] + rank : 0;
    __syncthreads();
    if (valid && rank == npeer - 1) base[d] += npeer;
    __syncthreads();
    if (valid && pos < n) {
      kout[pos] = key;
      vout[pos] = val;
    }
  }
}

// bstart[c], c = 0..ncell: the first position of the sorted cell ids holding an id >= c
__global__ void __launch_bounds__(256)
index_starts_kernel(const int *__restrict__ skeys, int n, int ncell, int *__restrict__ bstart) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c > ncell) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (skeys[mid] < (int)c) lo = mid + 1;
    else hi = mid;
  }
  bstart[c] = lo;
}

__global__ void __launch_bounds__(256)
index_fill_kernel(const float4 *__restrict__ ncoord, const int *__restrict__ svals, int n,
                  float4 *__restrict__ bxyz) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)n + kBinPad) return;
  float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the tail search_binned_kernel reads ahead into
  if (p < n) {
    const int i = svals[p];
    if ((unsigned)i < (unsigned)n) {  // always: svals is a permutation of 0..n-1
      o = ncoord[i];
      o.w = __int_as_float(i);
    }
  }
  bxyz[p] = o;
}

// index_fill_kernel for slots in cell order: point p carries its own position
__global__ void __launch_bounds__(256)
index_fill_pos_kernel(const float4 *__restrict__ ncoord, const int *__restrict__ svals, int n,
                      float4 *__restrict__ bxyz) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)n + kBinPad) return;
  float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (p < n) {
    const int i = svals[p];
    if ((unsigned)i < (unsigned)n) {  // always: svals is a permutation of 0..n-1
      o = ncoord[i];
      o.w = __int_as_float((int)p);
    }
  }
  bxyz[p] = o;
}

// order is a permutation of 0..n-1: every rank[] entry is written once, by one thread
__global__ void __launch_bounds__(256)
index_rank_kernel(const int *__restrict__ order, int n, int *__restrict__ rank) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int i = order[p];
  if ((unsigned)i < (unsigned)n) rank[i] = (int)p;
}

__global__ void __launch_bounds__(256)
index_compose_kernel(const int *__restrict__ ind, const int *__restrict__ rank, int n,
                     int *__restrict__ ind2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int o = ind[i];
  ind2[i] = (unsigned)o < (unsigned)n ? rank[o] : 0;  // always: ind is a permutation of 0..n-1
}

}  // namespace

int index_bound_blocks(int n) {
  return (int)std::min<long long>(std::max<long long>(((long long)n + kBoundThreads - 1) / kBoundThreads, 1), 1024);
}

hipError_t launch_index_normalize(hipStream_t s, const float *xyz, int n, int dim, float hinv,
                                  float vinv, float4 *ncoord, float *part) {
  hipLaunchKernelGGL(index_normalize_kernel, dim3(index_bound_blocks(n)), dim3(kBoundThreads), 0,
                     s, xyz, n, dim, hinv, vinv, ncoord, part);
  return hipGetLastError();
}

void index_finish_bounds(const float *part, int nblocks, IndexBounds &b) {
  float r[kIndexBoundWords];
  for (int j = 0; j < kIndexBoundWords; ++j) {
    const bool is_min = j < 3 || (j >= 6 && j < 9);
    r[j] = is_min ? INFINITY : -INFINITY;
    for (int k = 0; k < nblocks; ++k) {
      const float v = part[(size_t)k * kIndexBoundWords + j];
      r[j] = is_min ? std::min(r[j], v) : std::max(r[j], v);
    }
  }
  for (int c = 0; c < 3; ++c) {
    const bool seen = r[c] <= r[3 + c];  // unseen: +inf > -inf
    b.lo[c] = seen ? r[c] : 0.0f;
    b.hi[c] = seen ? r[3 + c] : 0.0f;
    b.alo[c] = r[6 + c];
    b.ahi[c] = r[9 + c];
  }
  b.aseen = r[6] <= r[9];
  if (!b.aseen)
    for (int c = 0; c < 3; ++c) b.alo[c] = b.ahi[c] = 0.0f;
}

int index_sort_blocks(int n) { return (n + kSortChunk - 1) / kSortChunk; }

hipError_t launch_index_sort(hipStream_t s, int n, int ncell, const float4 *ncoord, int dim,
                             IndexGrid g, int *keys[2], int *vals[2], int *hist, int *which) {
  *which = 0;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(index_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     ncoord, n, dim, g, keys[0], vals[0]);
  int bits = 0;
  while (bits < 31 && (1LL << bits) < ncell) ++bits;
  const int nblk = index_sort_blocks(n);
  int cur = 0;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(index_radix_hist_kernel, dim3(nblk), dim3(64), 0, s, keys[cur], n, shift,
                       nblk, hist);
    hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(1024), 0, s, hist, 256 * nblk);
    hipLaunchKernelGGL(index_radix_scatter_kernel, dim3(nblk), dim3(64), 0, s, keys[cur],
                       vals[cur], n, shift, nblk, hist, keys[cur ^ 1], vals[cur ^ 1]);
    cur ^= 1;
  }
  *which = cur;
  return hipGetLastError();
}

hipError_t launch_index_finish(hipStream_t s, const float4 *ncoord, int n, int ncell,
                               const int *skeys, const int *svals, float4 *bxyz, int *bstart,
                               bool by_position) {
  hipLaunchKernelGGL(index_starts_kernel, dim3((unsigned)((ncell + 1 + 255) / 256)), dim3(256), 0,
                     s, skeys, n, ncell, bstart);
  if (bxyz && by_position)
    hipLaunchKernelGGL(index_fill_pos_kernel, dim3((unsigned)((n + kBinPad + 255) / 256)),
                       dim3(256), 0, s, ncoord, svals, n, bxyz);
  else if (bxyz)
    hipLaunchKernelGGL(index_fill_kernel, dim3((unsigned)((n + kBinPad + 255) / 256)), dim3(256),
                       0, s, ncoord, svals, n, bxyz);
  return hipGetLastError();
}

hipError_t launch_index_rank(hipStream_t s, const int *order, int n, int *rank) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(index_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, order,
                     n, rank);
  return hipGetLastError();
}

hipError_t launch_index_compose(hipStream_t s, const int *ind, const int *rank, int n, int *ind2) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(index_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     ind, rank, n, ind2);
  return hipGetLastError();
}

}  // namespace cwbl
