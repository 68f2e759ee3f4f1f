// Nodes of a raster inside a buffered polygon set (reference data_prep.py:582-616, "Subset tiles to those within grounding line":
// the window boxes `within` the grounding line buffered by 10 km).  The selection is this project's own, defined exactly at the raster's
// nodes (include/dbm.h): even-odd parity of a ray to the east over ALL edges, and the closed Euclidean distance to the
// nearest edge against |buffer|.  Both are order-independent (a parity and an "any"), every quantity is float64 with one rounding per
// operation, so the mask is a function of the set of edges: the same bytes from call to call, under any permutation of the edges and
// on either schedule below.  No float atomics; integer atomics place list entries (the order inside a list is never visible).
//   cull     : one pass over the edges.  *proximity* list = edges whose box, grown by |buffer| + margin, meets the extent of the nodes;
//              *parity* list = edges that are not horizontal, whose y-span meets the rows and whose larger x (+ margin) is not west of
//              every node.  The same pass counts, per node tile of DBM_POLY_TILE^2 and per band of tile rows, the entries binning would
//              make, flags non-finite coordinates (the call is then refused before anything is written) and coordinates beyond 2^480
//              ("wild": the margins below assume no overflow, so such a call runs every edge against every node without shortcuts).
//   bin      : exclusive scan of the counts (three kernels, the scan of data_prims.h), then the lists are filled by tile / band.
//   classify : one 256-thread workgroup per tile, one node per thread.  DBM_POLY_CHUNK edges at a time are staged into LDS by 16-byte
//              loads (an edge is two of them; lanes 2k, 2k + 1 read the two halves of one edge) and every lane then reads the same LDS
//              address per edge (a broadcast: no bank conflict).  Proximity first; a wavefront whose nodes are all near has its answer
//              for either sign of the buffer and stops computing; the workgroup leaves a loop when all its wavefronts have.  Then the
//              parity, with a shortcut: a node west (east) of the edge's x-span by more than the margin crosses (does not cross) --
//              only nodes within the span evaluate the division.  One store per node.
//              Unbinned (the bins would exceed workspace_limit, or a wild call): the same kernel body, every tile ranging over the whole
//              culled lists (or over all edges).
// The margin.  With M = the largest magnitude among the edge's coordinates, the nodes' coordinates and |buffer|, every intermediate of d2
// (px, py, ex, ey, t ex, t ey, qx, qy) carries an absolute error of a few 2^-53 M: at most ~2^-49 M on qx and qy together, also when
// px - t ex cancels.  A node outside the edge's box grown by R = |buffer| + m is farther than R from the segment, so the computed
// sqrt(d2) > |buffer| + m - 2^-49 M, and with m = 2^-30 M (+ 2^-480, which covers squares that underflow) d2 > buffer^2 with 2^19 to
// spare: the edge can be dropped for that node, that tile, that raster.  For the parity the computed abscissa xa + ((y - ya) ex) / ey
// lies within a few 2^-53 M of [min(xa, xb), max(xa, xb)] whenever the row straddles the edge (|y - ya| <= |ey| after rounding, because
// rounding is monotone), so the same m decides nodes that far outside the span.
#include "model.h"
#include "data_layouts.h"
#include <cmath>

// the restatement rounds every difference, product, quotient and sum: nothing may be contracted into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int PT = DBM_POLY_TILE;
constexpr int POLY_THREADS = PT * PT;
constexpr int POLY_CHUNK = DBM_POLY_CHUNK;
constexpr int POLY_MAX_BLOCKS = 4096;    // grid-stride launches over the edges
constexpr int SCAN_ITEMS = 8;            // consecutive counts per lane of the scan kernels
constexpr int SCAN_TILE = POLY_THREADS * SCAN_ITEMS;
constexpr int NEAR_CHECK = 32;           // edges between two looks at "is the whole wavefront near"
constexpr double WILD = 0x1p480;
typedef unsigned long long u64;
static_assert(POLY_THREADS == 256 && POLY_CHUNK % NEAR_CHECK == 0 && (2 * POLY_CHUNK) % POLY_THREADS == 0, "staging shape");

struct Edge {
  double xa, ya, xb, yb;
};
struct Span {   // a closed box, or the rows / columns an edge may touch
  double x0, x1, y0, y1;
};

inline int stride_blocks(long n) { return grid_stride_blocks(n, POLY_THREADS, POLY_MAX_BLOCKS); }

__device__ inline double node(double o, double d, long i) { return o + (double)i * d; }   // one product, one sum, each rounded

__device__ inline double edge_margin(const Edge& e, double gmag) {
  const double m = fmax(fmax(fmax(fabs(e.xa), fabs(e.xb)), fmax(fabs(e.ya), fabs(e.yb))), gmag);
  return m * 0x1p-30 + 0x1p-480;
}

// the edge's box grown by |buffer| + margin; false: it misses the nodes' extent
__device__ inline bool prox_box(const PolyLaunch& a, const Edge& e, Span* b) {
  const double R = fabs(a.buffer) + edge_margin(e, a.gmag);
  b->x0 = fmin(e.xa, e.xb) - R;
  b->x1 = fmax(e.xa, e.xb) + R;
  b->y0 = fmin(e.ya, e.yb) - R;
  b->y1 = fmax(e.ya, e.yb) + R;
  return !(b->x1 < a.gx0 || b->x0 > a.gx1 || b->y1 < a.gy0 || b->y0 > a.gy1);
}

// can a node (x >= gx0, a row in [gy0, gy1]) count a crossing of the edge?
__device__ inline bool parity_keep(const PolyLaunch& a, const Edge& e) {
  return e.ya != e.yb && fmin(e.ya, e.yb) <= a.gy1 && a.gy0 < fmax(e.ya, e.yb) && fmax(e.xa, e.xb) + edge_margin(e, a.gmag) >= a.gx0;
}

// indices i in [0, n) whose node o + i d can lie in [lo, hi], widened by one on either side (the quotients are rounded); empty: *i0 > *i1
__device__ inline void axis_range(double lo, double hi, double o, double d, long n, long* i0, long* i1) {
  double p = (lo - o) / d, q = (hi - o) / d;
  if (p > q) { const double t = p; p = q; q = t; }
  p = floor(p) - 1.0;
  q = ceil(q) + 1.0;
  if (!(q >= 0.0) || !(p <= (double)(n - 1))) { *i0 = 1; *i1 = 0; return; }
  *i0 = p < 0.0 ? 0 : (long)p;
  *i1 = q > (double)(n - 1) ? n - 1 : (long)q;
}

// f(tile) for every node tile whose nodes' box meets b (exact comparisons on the tile's computed node coordinates)
template <class F>
__device__ inline void prox_tiles(const PolyLaunch& a, const Span& b, F f) {
  long c0, c1, r0, r1;
  axis_range(b.x0, b.x1, a.x0, a.dx, a.W, &c0, &c1);
  axis_range(b.y0, b.y1, a.y0, a.dy, a.H, &r0, &r1);
  if (c0 > c1 || r0 > r1) return;
  for (long ty = r0 / PT; ty <= r1 / PT; ++ty) {
    const long ra = ty * PT, rb = ra + PT - 1 < a.H ? ra + PT - 1 : a.H - 1;
    const double ya = node(a.y0, a.dy, ra), yb = node(a.y0, a.dy, rb);
    if (b.y1 < fmin(ya, yb) || b.y0 > fmax(ya, yb)) continue;
    for (long tx = c0 / PT; tx <= c1 / PT; ++tx) {
      const long ca = tx * PT, cb = ca + PT - 1 < a.W ? ca + PT - 1 : a.W - 1;
      const double xa = node(a.x0, a.dx, ca), xb = node(a.x0, a.dx, cb);
      if (b.x1 < fmin(xa, xb) || b.x0 > fmax(xa, xb)) continue;
      f(ty * a.tiles_x + tx);
    }
  }
}

// f(band) for every band of tile rows that holds a row y with min(ya, yb) <= y < max(ya, yb), judged on the band's first and last row
template <class F>
__device__ inline void parity_bands(const PolyLaunch& a, const Edge& e, F f) {
  const double lo = fmin(e.ya, e.yb), hi = fmax(e.ya, e.yb);
  long r0, r1;
  axis_range(lo, hi, a.y0, a.dy, a.H, &r0, &r1);
  if (r0 > r1) return;
  for (long ty = r0 / PT; ty <= r1 / PT; ++ty) {
    const long ra = ty * PT, rb = ra + PT - 1 < a.H ? ra + PT - 1 : a.H - 1;
    const double ya = node(a.y0, a.dy, ra), yb = node(a.y0, a.dy, rb);
    if (lo <= fmax(ya, yb) && fmin(ya, yb) < hi) f(ty);
  }
}

// totals: [0] proximity list, [1] parity list, [2] non-finite edges, [3] wild edges, [4] / [5] entries the tile / band bins would hold
__global__ __launch_bounds__(POLY_THREADS) void poly_cull_kernel(PolyLaunch a) {
  const long stride = (long)gridDim.x * POLY_THREADS;
  u64 binP = 0ull, binB = 0ull;
  const long bands0 = a.tiles_x * a.tiles_y;
  for (long i0 = (long)blockIdx.x * POLY_THREADS; i0 < a.n; i0 += stride) {   // (uniform per workgroup: the ballots need whole wavefronts)
    const long i = i0 + threadIdx.x;
    bool keepP = false, keepB = false;
    if (i < a.n) {
      const double* p = a.edges + 4 * i;
      const Edge e = {p[0], p[1], p[2], p[3]};
      const double big = fmax(fmax(fabs(e.xa), fabs(e.xb)), fmax(fabs(e.ya), fabs(e.yb)));
      if (!(isfinite(e.xa) && isfinite(e.ya) && isfinite(e.xb) && isfinite(e.yb))) {
        atomicAdd(&a.totals[2], 1ull);
      } else if (big > WILD) {
        atomicAdd(&a.totals[3], 1ull);
      } else {
        Span b;
        keepP = prox_box(a, e, &b);
        if (keepP) prox_tiles(a, b, [&](long t) { atomicAdd(&a.cnt[t], 1u); ++binP; });
        keepB = parity_keep(a, e);
        if (keepB) parity_bands(a, e, [&](long t) { atomicAdd(&a.cnt[bands0 + t], 1u); ++binB; });
      }
    }
    const u64 atP = wave_append(keepP, &a.totals[0]), atB = wave_append(keepB, &a.totals[1]);
    if (keepP) a.listP[atP] = (unsigned)i;
    if (keepB) a.listB[atB] = (unsigned)i;
  }
  if (binP) atomicAdd(&a.totals[4], binP);
  if (binB) atomicAdd(&a.totals[5], binB);
}

// ---- exclusive scan of cnt[0 .. nbins) into off (and cursor), off[nbins] = the sum ----
__device__ inline unsigned tile_counts(const PolyLaunch& a, unsigned* k) {
  return scan_tile_items<POLY_THREADS, SCAN_ITEMS, unsigned>(a.cnt, a.nbins, k, [](unsigned c) { return c; });
}

__global__ __launch_bounds__(POLY_THREADS) void poly_scan_sums_kernel(PolyLaunch a) {
  unsigned k[SCAN_ITEMS], tot;
  block_exscan<POLY_THREADS>(tile_counts(a, k), &tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(POLY_THREADS) void poly_scan_parts_kernel(PolyLaunch a, long tiles) {
  const unsigned sum = scan_parts<POLY_THREADS>(a.part, tiles);
  if (threadIdx.x == 0) a.off[a.nbins] = sum;
}

__global__ __launch_bounds__(POLY_THREADS) void poly_scan_offsets_kernel(PolyLaunch a) {
  const long first = scan_tile_first<POLY_THREADS, SCAN_ITEMS>();
  unsigned k[SCAN_ITEMS], tot;
  unsigned ex = block_exscan<POLY_THREADS>(tile_counts(a, k), &tot) + a.part[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    if (first + j < a.nbins) {
      a.off[first + j] = ex;
      a.cursor[first + j] = ex;
    }
    ex += k[j];
  }
}

// the culled lists, re-binned exactly as the cull pass counted them
__global__ __launch_bounds__(POLY_THREADS) void poly_fill_kernel(PolyLaunch a) {
  const long stride = (long)gridDim.x * POLY_THREADS, total = (long)a.nP + (long)a.nB, bands0 = a.tiles_x * a.tiles_y;
  for (long j = (long)blockIdx.x * POLY_THREADS + threadIdx.x; j < total; j += stride) {
    const bool prox = j < (long)a.nP;
    const unsigned i = prox ? a.listP[j] : a.listB[j - (long)a.nP];
    const double* p = a.edges + 4 * (long)i;
    const Edge e = {p[0], p[1], p[2], p[3]};
    if (prox) {
      Span b;
      if (prox_box(a, e, &b)) prox_tiles(a, b, [&](long t) { a.entries[atomicAdd(&a.cursor[t], 1u)] = i; });
    } else {
      parity_bands(a, e, [&](long t) { a.entries[atomicAdd(&a.cursor[bands0 + t], 1u)] = i; });
    }
  }
}

// ---- classify ----
// edges list[begin .. begin + n) (list == null: the edges begin .. themselves) into LDS, two 16-byte pieces per edge
__device__ inline void stage_edges(const PolyLaunch& a, const unsigned* __restrict__ list, long begin, int n, double2* sh) {
  const double2* src = (const double2*)a.edges;
#pragma unroll
  for (int p = threadIdx.x; p < 2 * POLY_CHUNK; p += POLY_THREADS) {
    const int k = p >> 1;
    if (k < n) {
      const long i = list ? (long)list[begin + k] : begin + k;
      sh[p] = src[2 * i + (p & 1)];
    }
  }
}

__global__ __launch_bounds__(POLY_THREADS) void poly_classify_kernel(PolyLaunch a) {
  __shared__ double2 sh[2 * POLY_CHUNK];
  const long tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const long r = ty * PT + (threadIdx.x >> 4), c = tx * PT + (threadIdx.x & 15);
  const bool valid = r < a.H && c < a.W;
  const double x = node(a.x0, a.dx, c), y = node(a.y0, a.dy, r);
  const double b2 = a.buffer * a.buffer;

  const unsigned *listP = a.listP, *listB = a.listB;
  long beginP = 0, endP = a.nP, beginB = 0, endB = a.nB;
  if (a.identity) {
    listP = listB = nullptr;
    endP = endB = a.n;
  } else if (a.entries) {
    listP = listB = a.entries;
    beginP = a.off[tile];
    endP = a.off[tile + 1];
    beginB = a.off[a.tiles_x * a.tiles_y + ty];
    endB = a.off[a.tiles_x * a.tiles_y + ty + 1];
  }

  // proximity: near = some edge has d2 <= buffer^2
  bool near = !valid;   // (a lane outside the raster never holds its wavefront back)
  bool wave_done = __all(near);
  for (long base = beginP; base < endP; base += POLY_CHUNK) {
    const int n = (int)(endP - base < POLY_CHUNK ? endP - base : POLY_CHUNK);
    stage_edges(a, listP, base, n, sh);
    __syncthreads();
    for (int k0 = 0; k0 < n && !wave_done; k0 += NEAR_CHECK) {
      const int k1 = k0 + NEAR_CHECK < n ? k0 + NEAR_CHECK : n;
      for (int k = k0; k < k1; ++k) {
        const double2 pa = sh[2 * k], pb = sh[2 * k + 1];
        const double ex = pb.x - pa.x, ey = pb.y - pa.y, px = x - pa.x, py = y - pa.y, L = ex * ex + ey * ey;
        double t = L > 0.0 ? (px * ex + py * ey) / L : 0.0;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double qx = px - t * ex, qy = py - t * ey, d2 = qx * qx + qy * qy;
        near = near || d2 <= b2;
      }
      wave_done = __all(near);
    }
    if (__syncthreads_or(!wave_done) == 0) break;   // (also: the chunk is free for the next staging)
  }
  near = near && valid;

  // parity of the crossings of the ray to the east; a wavefront that is all near has its answer for either sign of the buffer
  bool odd = false;
  if (__syncthreads_or(!wave_done) != 0) {
    for (long base = beginB; base < endB; base += POLY_CHUNK) {
      const int n = (int)(endB - base < POLY_CHUNK ? endB - base : POLY_CHUNK);
      stage_edges(a, listB, base, n, sh);
      __syncthreads();
      if (!wave_done) {
        for (int k = 0; k < n; ++k) {
          const double2 pa = sh[2 * k], pb = sh[2 * k + 1];
          if ((pa.y <= y) != (pb.y <= y)) {
            const Edge e = {pa.x, pa.y, pb.x, pb.y};
            const double m = edge_margin(e, a.gmag);
            bool cross;
            if (!a.identity && x < fmin(pa.x, pb.x) - m) cross = true;
            else if (!a.identity && x > fmax(pa.x, pb.x) + m) cross = false;
            else cross = x < pa.x + ((y - pa.y) * (pb.x - pa.x)) / (pb.y - pa.y);
            odd = odd != cross;
          }
        }
      }
      __syncthreads();
    }
  }
  if (!valid) return;
  const bool in = a.buffer >= 0.0 ? (odd || near) : (odd && !near);
  const long at = r * a.W + c;
  if (a.mask) a.mask[at] = in ? 1 : 0;
  if (a.grid && !in) a.grid[at] = __builtin_nanf("");
}

inline long scan_tiles(long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

}  // namespace

void polygon_geometry(PolyLaunch& a) {
  a.tiles_x = (a.W + PT - 1) / PT;
  a.tiles_y = (a.H + PT - 1) / PT;
  a.nbins = a.tiles_x * a.tiles_y + a.tiles_y;
  // the same two roundings as the kernels' node(): this translation unit is compiled with contraction off
  const double xe = a.x0 + (double)(a.W - 1) * a.dx, ye = a.y0 + (double)(a.H - 1) * a.dy;
  a.gx0 = std::fmin(a.x0, xe);
  a.gx1 = std::fmax(a.x0, xe);
  a.gy0 = std::fmin(a.y0, ye);
  a.gy1 = std::fmax(a.y0, ye);
  a.gmag = std::fmax(std::fmax(std::fmax(std::fabs(a.gx0), std::fabs(a.gx1)), std::fmax(std::fabs(a.gy0), std::fabs(a.gy1))), std::fabs(a.buffer));
  a.identity = !(a.gmag <= WILD) ? 1 : 0;
}

// the one layout of the workspace; *staged = room for a host table of edges (32 bytes each) if asked for, else null
size_t polygon_layout(PolyLaunch& a, bool stage_edges_too, double** staged, Carver c) {
  a.totals = c.take<u64>(8);
  a.listP = c.take<unsigned>((size_t)a.n);
  a.listB = c.take<unsigned>((size_t)a.n);
  a.cnt = c.take<unsigned>((size_t)a.nbins);
  a.cursor = c.take<unsigned>((size_t)a.nbins);
  a.off = c.take<unsigned>((size_t)(a.nbins + 1));
  a.part = c.take<unsigned>((size_t)scan_tiles(a.nbins));
  *staged = stage_edges_too ? c.take<double>(4 * (size_t)a.n) : nullptr;
  return c.bytes();
}

size_t polygon_workspace(const PolyLaunch& a, bool stage_edges_too) { PolyLaunch b = a; double* e; return polygon_layout(b, stage_edges_too, &e, Carver(nullptr)); }

double* polygon_carve(PolyLaunch& a, void* ws, bool stage_edges_too) { double* e; polygon_layout(a, stage_edges_too, &e, Carver(ws)); return e; }

void launch_polygon_cull(const PolyLaunch& a, hipStream_t s) {
  DBM_HIP(hipMemsetAsync(a.totals, 0, sizeof(u64) * 8, s));
  DBM_HIP(hipMemsetAsync(a.cnt, 0, 4 * (size_t)a.nbins, s));
  if (a.n > 0) hipLaunchKernelGGL(poly_cull_kernel, dim3(stride_blocks(a.n)), dim3(POLY_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_polygon_bin(const PolyLaunch& a, hipStream_t s) {
  const long tiles = scan_tiles(a.nbins);
  hipLaunchKernelGGL(poly_scan_sums_kernel, dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, a);
  hipLaunchKernelGGL(poly_scan_parts_kernel, dim3(1), dim3(POLY_THREADS), 0, s, a, tiles);
  hipLaunchKernelGGL(poly_scan_offsets_kernel, dim3((unsigned)tiles), dim3(POLY_THREADS), 0, s, a);
  if (a.nP + a.nB > 0u) hipLaunchKernelGGL(poly_fill_kernel, dim3(stride_blocks((long)a.nP + (long)a.nB)), dim3(POLY_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_polygon_classify(const PolyLaunch& a, hipStream_t s) {
  hipLaunchKernelGGL(poly_classify_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y)), dim3(POLY_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}
