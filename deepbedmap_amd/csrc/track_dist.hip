// The distribution of the along-track errors (reference deepbedmap.py:550-563, `df.describe()` of error = z_interpolated - z, and
// :575-608, `df.hist(column="error", bins=25)`): exact quantiles and a uniform-bin histogram of the errors of one dbm_grid_track call,
// from the points table (n, 3) and the z_interpolated column it wrote.  e_i = z_interpolated_i - z_i is formed on the fly in float64; an
// error takes part iff it is finite (the set dbm_grid_track reduces) and -0.0 counts as +0.0.  Semantics: DESIGN.md "Error distribution".
//   - Quantiles: a device-wide radix select.  Errors map to order-preserving 64-bit keys; eight passes fix one 8-bit digit each, from the
//     top.  In a pass every workgroup reads its grid-stride share of the points once and counts, for every wanted rank, the digit of the
//     keys that match the rank's prefix so far (ranks with one prefix share a histogram: in the first pass all of them, and its total is
//     m, the number of finite errors); one workgroup then narrows every rank's prefix with block_exscan.  The ranks are the two
//     neighbours of NumPy's method="linear" (h = (m - 1) q, j = floor(h)); the last pass turns them into a + d g (b - d (1 - g) where
//     g >= 0.5), d = b - a, each product and sum rounded on its own (NumPy fuses nothing).
//   - Histogram: `np.histogram(e, bins=B, range=(edges[0], edges[B]))`'s rule with the caller's B + 1 edges, counted per workgroup in LDS.
// Only integer atomics carry counts across lanes and workgroups, so every result is exact and the same bytes from call to call.
#include "model.h"
#include "data_prims.h"
#include <cmath>

// NumPy rounds every product and sum on its own; hipcc would contract a + d * g into a fused multiply-add in device code (and does so
// through __dmul_rn / __dadd_rn too, which are plain operators in HIP)
#pragma clang fp contract(off)

namespace {

constexpr int TD_THREADS = DBM_TRACK_DIST_THREADS;   // 256 = the digits of one pass: thread d of the narrowing workgroup owns digit d
constexpr int TD_MAX_BLOCKS = DBM_TRACK_DIST_BLOCKS;   // 4 workgroups per CU (32 KB of LDS each)
constexpr int TD_RANKS = 2 * DBM_TRACK_MAX_QUANTILES;   // two neighbouring order statistics per probability
constexpr int TD_PASSES = 8;
constexpr int TD_MAX_BINS = DBM_TRACK_MAX_BINS;
static_assert(TD_THREADS == 256, "one thread per digit");

typedef unsigned long long u64;

struct Probabilities {   // by value: the launch carries them
  double q[DBM_TRACK_MAX_QUANTILES];
  int count;
};

struct SelectState {     // between the passes, in the workspace
  u64 prefix[TD_RANKS];        // the digits fixed so far, highest first
  u64 below[TD_RANKS];         // the wanted rank among the keys that carry the prefix
  int slot[TD_RANKS];          // the histogram the rank counts in
  u64 slot_prefix[TD_RANKS];   // the prefix of each histogram in use
  int nslot;
  u64 m;                       // finite errors
};

// the error of point i as an order-preserving key; false: not finite, takes no part
__device__ __forceinline__ bool error_of(const TrackErrors& a, long i, double* e) {
  const double v = a.z_interp[i] - a.points[3 * i + 2];
  *e = v == 0.0 ? 0.0 : v;   // (-0.0 -> +0.0)
  return isfinite(v);
}
__device__ __forceinline__ u64 key_of(double e) {
  const u64 b = (u64)__double_as_longlong(e);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double value_of(u64 key) {
  return __longlong_as_double((long long)((key >> 63) ? (key ^ (1ull << 63)) : ~key));
}

// pass p counts digit (key >> (56 - 8 p)) & 255 of the keys whose higher digits equal a histogram's prefix
__global__ __launch_bounds__(TD_THREADS) void select_count_kernel(TrackErrors a, int pass, const SelectState* __restrict__ st,
                                                                  u64* __restrict__ hist) {
  __shared__ unsigned cnt[TD_RANKS * 256];   // (a workgroup's share stays below 2^32 keys: the entry point bounds n)
  __shared__ u64 pre[TD_RANKS];
  const int nslot = pass == 0 ? 1 : (st->nslot < TD_RANKS ? st->nslot : TD_RANKS);
  for (int j = threadIdx.x; j < nslot * 256; j += TD_THREADS) cnt[j] = 0u;
  if (pass > 0 && (int)threadIdx.x < nslot) pre[threadIdx.x] = st->slot_prefix[threadIdx.x];
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const long stride = (long)gridDim.x * TD_THREADS;
  for (long i = (long)blockIdx.x * TD_THREADS + threadIdx.x; i < a.n; i += stride) {
    double e;
    if (!error_of(a, i, &e)) continue;
    const u64 key = key_of(e);
    const int digit = (int)((key >> shift) & 255ull);
    if (pass == 0) {
      atomicAdd(&cnt[digit], 1u);
    } else {
      const u64 hi = key >> (shift + 8);
      for (int s = 0; s < nslot; ++s)
        if (hi == pre[s]) atomicAdd(&cnt[s * 256 + digit], 1u);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nslot * 256; j += TD_THREADS)
    if (cnt[j] != 0u) atomicAdd(&hist[j], (u64)cnt[j]);
}

// NumPy's method="linear" from the two neighbours a <= b of probability q among m values
__device__ inline double lerp_quantile(double a, double b, u64 m, double q) {
  const double top = (double)(m - 1), h = top * q;
  if (h >= top) return b;                        // both neighbours are the maximum
  const double g = h - floor(h), d = b - a;
  return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// One workgroup: every rank's prefix grows by the digit whose run of keys holds the rank; the histograms are left cleared for the
// next pass.  Pass 0 first reads m off the shared histogram and places the ranks; the last pass writes the quantiles.
__global__ __launch_bounds__(TD_THREADS) void select_narrow_kernel(int pass, Probabilities p, SelectState* __restrict__ st,
                                                                   u64* __restrict__ hist, double* __restrict__ out) {
  __shared__ SelectState s;
  __shared__ u64 nprefix[TD_RANKS], nbelow[TD_RANKS];
  const int t = threadIdx.x, nrank = 2 * p.count;
  if (pass == 0) {
    if (t < TD_RANKS) { s.prefix[t] = 0ull; s.below[t] = 0ull; s.slot[t] = 0; s.slot_prefix[t] = 0ull; }
    if (t == 0) { s.nslot = 1; s.m = 0ull; }
  } else {
    if (t < TD_RANKS) { s.prefix[t] = st->prefix[t]; s.below[t] = st->below[t]; s.slot[t] = st->slot[t]; }
    if (t == 0) { s.nslot = st->nslot < TD_RANKS ? st->nslot : TD_RANKS; s.m = st->m; }
  }
  __syncthreads();
  const int nslot = s.nslot;
  for (int sl = 0; sl < nslot; ++sl) {
    const u64 c = hist[sl * 256 + t];
    hist[sl * 256 + t] = 0ull;
    u64 total;
    const u64 ex = block_exscan<TD_THREADS>(c, &total);
    if (pass == 0) {   // (one histogram) total = m: rank 2 k is floor((m - 1) q_k), rank 2 k + 1 its upper neighbour
      if (t < nrank && total > 0ull) {
        const double top = (double)(total - 1ull), h = top * p.q[t >> 1];
        const u64 j = h >= top ? total - 1ull : (u64)floor(h) + (u64)(t & 1);
        s.below[t] = j < total ? j : total - 1ull;
      }
      if (t == 0) s.m = total;
      __syncthreads();
    }
    for (int r = 0; r < nrank; ++r)
      if (s.slot[r] == sl && c > 0ull && s.below[r] >= ex && s.below[r] - ex < c) {   // exactly one digit, if the histogram is not empty
        nprefix[r] = (s.prefix[r] << 8) | (u64)t;
        nbelow[r] = s.below[r] - ex;
      }
  }
  __syncthreads();
  if (t < nrank && s.m > 0ull) { s.prefix[t] = nprefix[t]; s.below[t] = nbelow[t]; }
  __syncthreads();
  if (t == 0) {   // ranks with one prefix count in one histogram
    int used = 0;
    for (int r = 0; r < nrank; ++r) {
      int at = 0;
      while (at < used && s.slot_prefix[at] != s.prefix[r]) ++at;
      if (at == used) s.slot_prefix[used++] = s.prefix[r];
      s.slot[r] = at;
    }
    s.nslot = used > 0 ? used : 1;
  }
  __syncthreads();
  if (pass + 1 < TD_PASSES) {
    if (t < TD_RANKS) { st->prefix[t] = s.prefix[t]; st->below[t] = s.below[t]; st->slot[t] = s.slot[t]; st->slot_prefix[t] = s.slot_prefix[t]; }
    if (t == 0) { st->nslot = s.nslot; st->m = s.m; }
  } else if (t < p.count) {   // the prefixes are whole keys now
    out[t] = s.m > 0ull ? lerp_quantile(value_of(s.prefix[2 * t]), value_of(s.prefix[2 * t + 1]), s.m, p.q[t]) : __builtin_nan("");
  }
}

__global__ __launch_bounds__(TD_THREADS) void error_histogram_kernel(TrackErrors a, const double* __restrict__ edges, int B,
                                                                     u64* __restrict__ counts) {
  __shared__ u64 cnt[TD_MAX_BINS];
  for (int j = threadIdx.x; j < B; j += TD_THREADS) cnt[j] = 0ull;
  __syncthreads();
  const double first = edges[0], last = edges[B], width = last - first;
  const long stride = (long)gridDim.x * TD_THREADS;
  for (long k = (long)blockIdx.x * TD_THREADS + threadIdx.x; k < a.n; k += stride) {
    double e;
    if (!error_of(a, k, &e) || !(e >= first && e <= last)) continue;
    long i = (long)(((e - first) / width) * (double)B);
    i = i < 0 ? 0 : (i > B - 1 ? B - 1 : i);   // (i == B: the right edge belongs to the last bin; the rest never leaves 0 .. B)
    if (e < edges[i] && i > 0) --i;            // the index may be off by one within an ulp of an edge
    if (e >= edges[i + 1] && i != B - 1) ++i;
    atomicAdd(&cnt[i], 1ull);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < B; j += TD_THREADS)
    if (cnt[j] != 0ull) atomicAdd(&counts[j], cnt[j]);
}

struct QuantileSpace { u64* hist; SelectState* state; };
QuantileSpace carve_quantiles(Carver& c) { return {c.take<u64>((size_t)TD_RANKS * 256), c.take<SelectState>(1)}; }

}  // namespace

size_t track_quantiles_workspace() {
  Carver c(nullptr);
  carve_quantiles(c);
  return c.bytes();
}

size_t track_histogram_workspace(int bins) { return align256(sizeof(double) * ((size_t)bins + 1)); }

static_assert(DBM_TRACK_DIST_WORKSPACE >= sizeof(u64) * TD_RANKS * 256 + ((sizeof(SelectState) + 255) & ~(size_t)255) &&
                  DBM_TRACK_DIST_WORKSPACE >= sizeof(double) * (TD_MAX_BINS + 1) + 255,
              "include/dbm.h promises a workspace both calls fit in");

void launch_track_error_quantiles(const TrackErrors& a, const double* probs, int count, double* out, void* ws, hipStream_t s) {
  Carver c(ws);
  const QuantileSpace w = carve_quantiles(c);
  Probabilities p;
  for (int k = 0; k < DBM_TRACK_MAX_QUANTILES; ++k) p.q[k] = k < count ? probs[k] : 0.0;
  p.count = count;
  DBM_HIP(hipMemsetAsync(w.hist, 0, sizeof(u64) * TD_RANKS * 256, s));
  const int blocks = grid_stride_blocks(a.n, TD_THREADS, TD_MAX_BLOCKS);
  for (int pass = 0; pass < TD_PASSES; ++pass) {
    hipLaunchKernelGGL(select_count_kernel, dim3(blocks), dim3(TD_THREADS), 0, s, a, pass, w.state, w.hist);
    hipLaunchKernelGGL(select_narrow_kernel, dim3(1), dim3(TD_THREADS), 0, s, pass, p, w.state, w.hist, out);
  }
  DBM_HIP(hipGetLastError());
}

void launch_track_error_histogram(const TrackErrors& a, const double* edges_host, int bins, long long* counts, void* ws, hipStream_t s) {
  double* edges = (double*)ws;
  DBM_HIP(hipMemcpyAsync(edges, edges_host, sizeof(double) * ((size_t)bins + 1), hipMemcpyHostToDevice, s));
  DBM_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)bins, s));
  hipLaunchKernelGGL(error_histogram_kernel, dim3(grid_stride_blocks(a.n, TD_THREADS, TD_MAX_BLOCKS)), dim3(TD_THREADS), 0, s, a, edges,
                     bins, (u64*)counts);
  DBM_HIP(hipGetLastError());
}
