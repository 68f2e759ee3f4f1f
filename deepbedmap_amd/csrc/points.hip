// Survey point clouds -> tables and grids (reference data_prep.py:322-334 the `filters.reprojection` step of ascii_to_xyz, :353-378
// get_region, :406-407 the `gmt.blockmedian` preprocessing of xyz_to_grid).  Three passes over float64 point tables (n, ncol) resident
// in HBM (DESIGN.md "Gridding point clouds"):
//   - projection: EPSG method 9829 variant B, south-pole case (EPSG:4326 -> EPSG:3031), one lane per row, constants from the host;
//   - region: min / max of x and y over the rows whose x, y[, z] are all finite, lane -> wave -> workgroup -> one finishing workgroup
//     (min and max are exact in any order; the launch depends on n only), outward to multiples of the increment;
//   - block medians: row -> block index, integer histogram, exclusive scan of the H W counts and of the non-empty flags (three kernels:
//     workgroup sums, one workgroup over the sums, rescan: data_prims.h), rows scattered block-contiguously with integer atomics (the order INSIDE a
//     block is arbitrary and never visible: every block is then sorted or selected from), medians per size class of population k:
//       k <= DBM_BLOCKMEDIAN_SUB8 : 8 lanes per block, 32 blocks per workgroup     } rank by counting across the lanes of a
//       k <= DBM_BLOCKMEDIAN_SUB32: 32 lanes per block, 8 blocks per workgroup     } sub-group (k shuffles per column): no LDS,
//       k <= DBM_BLOCKMEDIAN_WAVE : one wavefront per block, 4 per workgroup       } no barrier
//       k <= DBM_BLOCKMEDIAN_LDS  : one workgroup per block, bitonic sort of the 64-bit keys in 16 KiB of LDS
//       larger                    : one workgroup per block, radix select (8 passes of 8 bits per wanted rank) out of global memory
//     on the order-preserving 64-bit image of the doubles (a total order: -0.0 before +0.0, ties by lane), so the result is a function
//     of the multiset of rows.  No float atomics anywhere.
#include "model.h"
#include "data_layouts.h"
#include <cmath>

// NumPy rounds every quotient, sum and product: the block assignment may not be contracted into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int PTS_THREADS = DBM_POINTS_THREADS;
constexpr int PTS_MAX_BLOCKS = 4096;     // grid-stride launches: 16 workgroups per CU
constexpr int SCAN_ITEMS = 8;            // consecutive counts per lane of the scan kernels
constexpr int SCAN_TILE = PTS_THREADS * SCAN_ITEMS;
typedef unsigned long long u64;

inline int stride_blocks(long n) { return grid_stride_blocks(n, PTS_THREADS, PTS_MAX_BLOCKS); }

// ---- projection ----
__global__ __launch_bounds__(PTS_THREADS) void polar_stereographic_kernel(ProjLaunch a) {
  const long stride = (long)gridDim.x * PTS_THREADS;
  const double rad = 3.14159265358979323846 / 180.0;
  for (long i = (long)blockIdx.x * PTS_THREADS + threadIdx.x; i < a.n; i += stride) {
    const double* p = a.in + i * a.ncol;
    double* q = a.out + i * a.ncol;
    const double lon = p[0], lat = p[1];
    double E = __builtin_nan(""), N = E;
    if (isfinite(lon) && isfinite(lat)) {
      const double es = a.e * sin(lat * rad);
      // tan(pi/4 + phi/2) from degrees: 45 + phi/2 is exact at the pole (0) where the radian sum is not
      const double t = tan((45.0 + 0.5 * lat) * rad) / pow((1.0 + es) / (1.0 - es), a.half_e);
      const double rho = a.scale * t, dl = lon * rad - a.lon0;
      E = a.fe + rho * sin(dl);
      N = a.fn + rho * cos(dl);
    }
    if (q != p)
      for (int c = 2; c < a.ncol; ++c) q[c] = p[c];
    q[0] = E;
    q[1] = N;
  }
}

// ---- region ----
struct Box {
  double xmin, xmax, ymin, ymax;
  long long cnt;
};

__device__ inline Box box_merge(const Box& a, const Box& b) {
  return {fmin(a.xmin, b.xmin), fmax(a.xmax, b.xmax), fmin(a.ymin, b.ymin), fmax(a.ymax, b.ymax), a.cnt + b.cnt};
}

__global__ __launch_bounds__(PTS_THREADS) void region_kernel(const double* __restrict__ pts, long n, int ncol, Box* part) {
  Box m = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0};
  const long stride = (long)gridDim.x * PTS_THREADS;
  for (long i = (long)blockIdx.x * PTS_THREADS + threadIdx.x; i < n; i += stride) {
    const double* p = pts + i * ncol;
    const double x = p[0], y = p[1];
    if (isfinite(x) && isfinite(y) && (ncol < 3 || isfinite(p[2]))) {
      m.xmin = fmin(m.xmin, x);
      m.xmax = fmax(m.xmax, x);
      m.ymin = fmin(m.ymin, y);
      m.ymax = fmax(m.ymax, y);
      m.cnt += 1;
    }
  }
  m = block_reduce<PTS_THREADS>(m, box_merge);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// one workgroup folds the partials (fold_partials); region = the box moved outward to multiples of inc
__global__ __launch_bounds__(PTS_THREADS) void region_finish_kernel(const Box* __restrict__ part, int blocks, double inc, double* region,
                                                                    long long* count) {
  const Box r = fold_partials<PTS_THREADS>(blocks, Box{INFINITY, -INFINITY, INFINITY, -INFINITY, 0}, [part](long b) { return part[b]; }, box_merge);
  if (threadIdx.x != 0) return;
  const double nan = __builtin_nan("");
  const bool any = r.cnt > 0;
  region[0] = any ? floor(r.xmin / inc) * inc : nan;
  region[1] = any ? ceil(r.xmax / inc) * inc : nan;
  region[2] = any ? floor(r.ymin / inc) * inc : nan;
  region[3] = any ? ceil(r.ymax / inc) * inc : nan;
  *count = r.cnt;
}

// ---- block medians ----
// order-preserving image of a double: a < b (with -0.0 < +0.0) iff okey(a) < okey(b) as unsigned integers
__device__ inline u64 okey(double v) {
  const u64 u = (u64)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double okey_value(u64 k) {
  const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// blk[i] = block of row i (row-major from the north-west node) or -1; cnt[block] += 1
__global__ __launch_bounds__(PTS_THREADS) void bm_assign_kernel(BlockMedianLaunch a) {
  const long stride = (long)gridDim.x * PTS_THREADS;
  for (long i = (long)blockIdx.x * PTS_THREADS + threadIdx.x; i < a.n; i += stride) {
    const double* p = a.points + 3 * i;
    const double x = p[0], y = p[1], z = p[2];
    int b = -1;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      const double c = floor((x - a.xmin) / a.inc + 0.5), r = floor((a.ymax - y) / a.inc + 0.5);
      if (c >= 0.0 && c < (double)a.W && r >= 0.0 && r < (double)a.H) {
        b = (int)((long)r * a.W + (long)c);
        atomicAdd(&a.cnt[b], 1u);
      }
    }
    a.blk[i] = b;
  }
}

struct Pair {  // (points, non-empty blocks)
  unsigned s, f;
};

__device__ inline Pair operator+(Pair x, Pair y) { return {x.s + y.s, x.f + y.f}; }
__device__ inline Pair operator-(Pair x, Pair y) { return {x.s - y.s, x.f - y.f}; }

// the calling thread's SCAN_ITEMS consecutive counts of the tile into k; their (sum, number that are not zero)
__device__ inline Pair tile_counts(const BlockMedianLaunch& a, unsigned* k) {
  return scan_tile_items<PTS_THREADS, SCAN_ITEMS, Pair>(a.cnt, a.H * a.W, k, [](unsigned c) { return Pair{c, c != 0u ? 1u : 0u}; });
}

__global__ __launch_bounds__(PTS_THREADS) void bm_tile_sums_kernel(BlockMedianLaunch a) {
  unsigned k[SCAN_ITEMS];
  Pair tot;
  block_exscan<PTS_THREADS>(tile_counts(a, k), &tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = make_uint2(tot.s, tot.f);
}

// one workgroup: part[t] <- exclusive scan; totals[0] = non-empty blocks, off[H W] = points used, class counters cleared
__global__ __launch_bounds__(PTS_THREADS) void bm_scan_sums_kernel(BlockMedianLaunch a, long tiles) {
  const Pair sum = scan_parts<PTS_THREADS>((Pair*)a.part, tiles);
  if (threadIdx.x == 0) {
    a.totals[0] = sum.f;
    a.off[a.H * a.W] = sum.s;
  }
  if (threadIdx.x >= 1 && threadIdx.x <= DBM_BLOCKMEDIAN_CLASSES) a.totals[threadIdx.x] = 0u;
}

__device__ inline int size_class(unsigned k) {
  return k == 0u ? -1 : k <= DBM_BLOCKMEDIAN_SUB8 ? 0 : k <= DBM_BLOCKMEDIAN_SUB32 ? 1 : k <= DBM_BLOCKMEDIAN_WAVE ? 2 : k <= DBM_BLOCKMEDIAN_LDS ? 3 : 4;
}

// off[b], rowof[b] for every block; non-empty blocks appended to their size class's list (one atomic per wave and class: the order of
// a list is arbitrary, what is computed per block is not)
__global__ __launch_bounds__(PTS_THREADS) void bm_offsets_kernel(BlockMedianLaunch a) {
  const long hw = a.H * a.W, first = scan_tile_first<PTS_THREADS, SCAN_ITEMS>();
  unsigned k[SCAN_ITEMS];
  Pair tot;
  Pair ex = block_exscan<PTS_THREADS>(tile_counts(a, k), &tot) + ((const Pair*)a.part)[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const long b = first + j;
    if (b < hw) {
      a.off[b] = ex.s;
      a.rowof[b] = ex.f;
    }
    ex.s += k[j];
    ex.f += k[j] != 0u;
    const int cls = b < hw ? size_class(k[j]) : -1;
    for (int c = 0; c < DBM_BLOCKMEDIAN_CLASSES; ++c) {
      const unsigned at = wave_append(cls == c, &a.totals[1 + c]);
      if (cls == c) a.lists[c][at] = (unsigned)b;
    }
  }
}

// the optional rasters before anything is placed: counts = the histogram, grid = NaN (non-empty blocks are overwritten by the medians)
__global__ __launch_bounds__(PTS_THREADS) void bm_rasters_kernel(BlockMedianLaunch a) {
  const long hw = a.H * a.W, stride = (long)gridDim.x * PTS_THREADS;
  for (long b = (long)blockIdx.x * PTS_THREADS + threadIdx.x; b < hw; b += stride) {
    if (a.counts) a.counts[b] = (int)a.cnt[b];
    if (a.grid) a.grid[b] = __builtin_nanf("");
  }
}

// perm[off[b] .. off[b + 1]) = the rows of block b; the histogram counts down to zero while it hands out the places
__global__ __launch_bounds__(PTS_THREADS) void bm_scatter_kernel(BlockMedianLaunch a) {
  const long stride = (long)gridDim.x * PTS_THREADS;
  for (long i = (long)blockIdx.x * PTS_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int b = a.blk[i];
    if (b >= 0) a.perm[a.off[b] + atomicSub(&a.cnt[b], 1u) - 1u] = (unsigned)i;
  }
}

__device__ inline void bm_store(const BlockMedianLaunch& a, unsigned b, int c, double lo, double hi, bool two) {
  const double med = two ? 0.5 * (lo + hi) : lo;
  a.table[3 * (long)a.rowof[b] + c] = med;
  if (c == 2 && a.grid) a.grid[b] = (float)med;
}

// S lanes per block (k <= S): lane j of a sub-group holds row j; its rank = how many of the k keys sort before it (ties by lane)
template <int S>
__global__ __launch_bounds__(PTS_THREADS) void bm_subgroup_kernel(BlockMedianLaunch a, const unsigned* __restrict__ list, unsigned nlist) {
  static_assert(S >= 1 && S <= 64 && (S & (S - 1)) == 0, "a sub-group is a power-of-two slice of a wavefront");
  const int lane = threadIdx.x & 63, sub = lane % S, g0 = lane - sub;
  const unsigned unit = (unsigned)(((u64)blockIdx.x * PTS_THREADS + threadIdx.x) / S);
  const bool live = unit < nlist;
  unsigned b = 0u, k = 0u, o = 0u;
  if (live) {
    b = list[unit];
    o = a.off[b];
    k = a.off[b + 1] - o;
  }
  const bool have = (unsigned)sub < k;
  double v[3] = {0.0, 0.0, 0.0};
  if (have) {
    const double* p = a.points + 3 * (long)a.perm[o + sub];
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  }
  unsigned kmax = k;   // the wave's largest population bounds the (uniform) loop
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned other = __shfl_xor(kmax, off, 64);
    kmax = other > kmax ? other : kmax;
  }
  const unsigned rlo = (k - 1u) / 2u, rhi = k / 2u;
  for (int c = 0; c < 3; ++c) {
    const u64 key = okey(v[c]);
    unsigned rank = 0u;
    for (unsigned j = 0; j < kmax; ++j) {
      const u64 kj = __shfl(key, g0 + (int)j, 64);
      rank += (j < k && (kj < key || (kj == key && j < (unsigned)sub))) ? 1u : 0u;
    }
    u64 mlo = __ballot(have && rank == rlo), mhi = __ballot(have && rank == rhi);
    if constexpr (S < 64) {
      mlo = (mlo >> g0) & ((1ull << S) - 1ull);
      mhi = (mhi >> g0) & ((1ull << S) - 1ull);
    }
    const int slo = mlo ? g0 + __ffsll((long long)mlo) - 1 : g0, shi = mhi ? g0 + __ffsll((long long)mhi) - 1 : g0;
    const double lo = __shfl(v[c], slo, 64), hi = __shfl(v[c], shi, 64);
    if (live && sub == 0) bm_store(a, b, c, lo, hi, rlo != rhi);
  }
}

// one workgroup per block, k <= DBM_BLOCKMEDIAN_LDS: bitonic sort of the keys padded with ~0 (above every finite key) to a power of two
__global__ __launch_bounds__(PTS_THREADS) void bm_lds_kernel(BlockMedianLaunch a, const unsigned* __restrict__ list) {
  static_assert((DBM_BLOCKMEDIAN_LDS & (DBM_BLOCKMEDIAN_LDS - 1)) == 0, "the sort pads to a power of two");
  __shared__ u64 keys[DBM_BLOCKMEDIAN_LDS];
  const unsigned b = list[blockIdx.x], o = a.off[b], k = a.off[b + 1] - o;
  unsigned P = 2u;
  while (P < k) P <<= 1;
  for (int c = 0; c < 3; ++c) {
    for (unsigned i = threadIdx.x; i < P; i += PTS_THREADS) keys[i] = i < k ? okey(a.points[3 * (long)a.perm[o + i] + c]) : ~0ull;
    __syncthreads();
    for (unsigned size = 2u; size <= P; size <<= 1)
      for (unsigned stride = size >> 1; stride > 0u; stride >>= 1) {
        for (unsigned t = threadIdx.x; t < P / 2u; t += PTS_THREADS) {
          const unsigned i = 2u * t - (t & (stride - 1u)), j = i + stride;
          const u64 x = keys[i], y = keys[j];
          if ((x > y) == ((i & size) == 0u)) { keys[i] = y; keys[j] = x; }
        }
        __syncthreads();
      }
    if (threadIdx.x == 0) bm_store(a, b, c, okey_value(keys[(k - 1u) / 2u]), okey_value(keys[k / 2u]), (k & 1u) == 0u);
    __syncthreads();
  }
}

// the key of rank `rank` (0-based) among column c of rows perm[o .. o + k): eight passes fix eight bits each, from the top
__device__ u64 radix_select(const BlockMedianLaunch& a, unsigned o, unsigned k, int c, unsigned rank, unsigned* hist, unsigned* pick) {
  u64 prefix = 0ull, mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0u;   // (256 bins, 256 threads)
    __syncthreads();
    for (unsigned i = threadIdx.x; i < k; i += PTS_THREADS) {
      const u64 key = okey(a.points[3 * (long)a.perm[o + i] + c]);
      if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned d = 0u, r = rank;
      while (d < 255u && r >= hist[d]) r -= hist[d++];
      pick[0] = d;
      pick[1] = r;
    }
    __syncthreads();
    prefix |= (u64)pick[0] << shift;
    mask |= 0xffull << shift;
    rank = pick[1];
    __syncthreads();
  }
  return prefix;
}

__global__ __launch_bounds__(PTS_THREADS) void bm_global_kernel(BlockMedianLaunch a, const unsigned* __restrict__ list) {
  static_assert(PTS_THREADS == 256, "one histogram bin per thread");
  __shared__ unsigned hist[256], pick[2];
  const unsigned b = list[blockIdx.x], o = a.off[b], k = a.off[b + 1] - o;
  for (int c = 0; c < 3; ++c) {
    const u64 lo = radix_select(a, o, k, c, (k - 1u) / 2u, hist, pick);
    const u64 hi = (k & 1u) ? lo : radix_select(a, o, k, c, k / 2u, hist, pick);
    if (threadIdx.x == 0) bm_store(a, b, c, okey_value(lo), okey_value(hi), (k & 1u) == 0u);
  }
}

inline long scan_tiles(long hw) { return (hw + SCAN_TILE - 1) / SCAN_TILE; }
inline size_t list_capacity(int c, long n, long hw) {   // blocks that can hold more than `floor` points each
  const long floor_k[DBM_BLOCKMEDIAN_CLASSES] = {1, DBM_BLOCKMEDIAN_SUB8 + 1, DBM_BLOCKMEDIAN_SUB32 + 1, DBM_BLOCKMEDIAN_WAVE + 1, DBM_BLOCKMEDIAN_LDS + 1};
  const long cap = n / floor_k[c];
  return (size_t)(cap < hw ? cap : hw);
}

}  // namespace

void launch_points_project(const ProjLaunch& a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(polar_stereographic_kernel, dim3(stride_blocks(a.n)), dim3(PTS_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

size_t points_region_workspace(long n) { return align256(sizeof(Box) * (size_t)stride_blocks(n)); }

void launch_points_region(const double* pts, long n, int ncol, double inc, void* ws, double* region, long long* count, hipStream_t s) {
  const int blocks = stride_blocks(n);
  if (n > 0) {
    hipLaunchKernelGGL(region_kernel, dim3(blocks), dim3(PTS_THREADS), 0, s, pts, n, ncol, (Box*)ws);
    DBM_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(region_finish_kernel, dim3(1), dim3(PTS_THREADS), 0, s, (const Box*)ws, n > 0 ? blocks : 0, inc, region, count);
  DBM_HIP(hipGetLastError());
}

// the one layout of the block medians' workspace
size_t blockmedian_layout(BlockMedianLaunch& a, long n, long hw, Carver c) {
  a.blk = c.take<int>((size_t)n);
  a.perm = c.take<unsigned>((size_t)n);
  a.cnt = c.take<unsigned>((size_t)hw);
  a.rowof = c.take<unsigned>((size_t)hw);
  a.off = c.take<unsigned>((size_t)(hw + 1));
  a.part = c.take<uint2>((size_t)scan_tiles(hw));
  a.totals = c.take<unsigned>(1 + DBM_BLOCKMEDIAN_CLASSES);
  for (int k = 0; k < DBM_BLOCKMEDIAN_CLASSES; ++k) a.lists[k] = c.take<unsigned>(list_capacity(k, n, hw));
  return c.bytes();
}

size_t blockmedian_workspace(long n, long hw) { BlockMedianLaunch a; return blockmedian_layout(a, n, hw, Carver(nullptr)); }

void blockmedian_carve(BlockMedianLaunch& a, void* ws) { blockmedian_layout(a, a.n, a.H * a.W, Carver(ws)); }

void launch_blockmedian_count(const BlockMedianLaunch& a, hipStream_t s) {
  const long hw = a.H * a.W, tiles = scan_tiles(hw);
  DBM_HIP(hipMemsetAsync(a.cnt, 0, 4 * (size_t)hw, s));
  if (a.n > 0) hipLaunchKernelGGL(bm_assign_kernel, dim3(stride_blocks(a.n)), dim3(PTS_THREADS), 0, s, a);
  hipLaunchKernelGGL(bm_tile_sums_kernel, dim3((unsigned)tiles), dim3(PTS_THREADS), 0, s, a);
  hipLaunchKernelGGL(bm_scan_sums_kernel, dim3(1), dim3(PTS_THREADS), 0, s, a, tiles);
  hipLaunchKernelGGL(bm_offsets_kernel, dim3((unsigned)tiles), dim3(PTS_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_blockmedian_select(const BlockMedianLaunch& a, const unsigned* totals, hipStream_t s) {
  const long hw = a.H * a.W;
  if (a.grid || a.counts) hipLaunchKernelGGL(bm_rasters_kernel, dim3(stride_blocks(hw)), dim3(PTS_THREADS), 0, s, a);
  if (totals[0] > 0u) {
    hipLaunchKernelGGL(bm_scatter_kernel, dim3(stride_blocks(a.n)), dim3(PTS_THREADS), 0, s, a);
    const unsigned* t = totals + 1;
    constexpr int S0 = DBM_BLOCKMEDIAN_SUB8, S1 = DBM_BLOCKMEDIAN_SUB32, S2 = DBM_BLOCKMEDIAN_WAVE;   // blocks per workgroup: 256 / S
    if (t[0]) hipLaunchKernelGGL(bm_subgroup_kernel<S0>, dim3((t[0] + PTS_THREADS / S0 - 1) / (PTS_THREADS / S0)), dim3(PTS_THREADS), 0, s, a, a.lists[0], t[0]);
    if (t[1]) hipLaunchKernelGGL(bm_subgroup_kernel<S1>, dim3((t[1] + PTS_THREADS / S1 - 1) / (PTS_THREADS / S1)), dim3(PTS_THREADS), 0, s, a, a.lists[1], t[1]);
    if (t[2]) hipLaunchKernelGGL(bm_subgroup_kernel<S2>, dim3((t[2] + PTS_THREADS / S2 - 1) / (PTS_THREADS / S2)), dim3(PTS_THREADS), 0, s, a, a.lists[2], t[2]);
    if (t[3]) hipLaunchKernelGGL(bm_lds_kernel, dim3(t[3]), dim3(PTS_THREADS), 0, s, a, a.lists[3]);
    if (t[4]) hipLaunchKernelGGL(bm_global_kernel, dim3(t[4]), dim3(PTS_THREADS), 0, s, a, a.lists[4]);
  }
  DBM_HIP(hipGetLastError());
}
