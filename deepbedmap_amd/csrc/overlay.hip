// Vector layers on a resident image: line segments and discs painted in place (dbm_image_overlay, dbm_image_overlay_stats; the layer
// objects and the NumPy statement are deepbedmap_amd/overlay.py).  Reference: paper_figures.py:533-562 (Figure 2: `fig.coast(
// shorelines="0.25p")`, `fig.plot(style="r+s", pen="1p,orange2")` -- the grounding line, the study regions and the training tiles as
// boxes) and :1039-1045 (Figure 5a: `fig.plot(style="c0.1c", color="orange")` -- survey points on the DEM).  The rule is this project's
// own (include/dbm.h), not GMT's pixels: every pixel has S x S sub-samples, a sub-sample is covered if SOME primitive of
// the layer lies within size / 2 pixels of it (a closed comparison on float64 operations that are rounded once each), and the layer's
// colour is blended over the pixel with integer arithmetic by the number of covered sub-samples.  Coverage is an "any", so the bytes
// are a function of the set of primitives: the same from call to call, under any permutation and on either schedule below.  No float
// atomics; integer atomics place list entries (the order inside a list is never visible).
//   cull  : one grid-stride pass over the primitives.  Coordinates become pixel units, u = (x - x0) / dx, v = (y - y0) / dy; a primitive
//           with a non-finite coordinate is counted (the call is then refused before a byte is written); one whose pixel coordinates
//           overflowed covers nothing by the rule (every d2 is inf or NaN) and is dropped; one whose box of pixel centres (below)
//           misses the image is dropped.  The kept ones are appended, converted, to a compact table, and the pass sums the entries
//           the tile bins would hold: per primitive the number of OVERLAY_TILE^2 pixel tiles its box meets, a product.  The counts
//           per tile are made by a second pass only once the host knows that the bins fit workspace_limit, so the work of counting
//           is bounded by that limit whatever the size of the pen.
//   bin   : counts per tile, the exclusive scan of data_prims.h (three kernels), then the lists are filled tile by tile.
//   paint : one 256-thread workgroup per tile, one pixel per thread.  DBM_OVERLAY_CHUNK primitives at a time are staged into LDS by
//           16-byte loads (thread k stages primitive k and its box), and every lane then reads the same LDS address per primitive (a
//           broadcast: no bank conflict).  A lane whose pixel centre lies outside the primitive's box skips it; otherwise it evaluates
//           its S^2 sub-samples and ORs the covered ones into a mask of S^2 bits.  A lane whose mask is full skips the arithmetic, a
//           wavefront whose lanes are all full leaves the loop, the workgroup stops staging when all its wavefronts have.  Then a
//           popcount, the blend, one store per pixel; a pixel without a covered sub-sample is not stored.
//           Unbinned (the bins would exceed workspace_limit): the same kernel body, every tile ranging over the whole compact table.
// The margin.  Sub-sample coordinates are exact: c + ((j + 1/2) / S - 1/2) with S a power of two.  With M = the largest magnitude
// among the primitive's pixel coordinates, W, H and the radius r = size / 2, every intermediate of d2 (px, py, ex, ey, t ex, t ey, qx,
// qy) carries an absolute error of a few 2^-53 M: at most ~2^-49 M on qx and qy together, whatever t in [0, 1] the clamped division
// gave (also when L overflowed and t = 0: the point at t lies on the segment).  A sub-sample outside the primitive's box grown by
// r + m is farther than r + m from the segment, so the computed sqrt(d2) > r + m - 2^-49 M, and with m = 2^-30 M (+ 2^-480, which
// covers squares that underflow) d2 > r^2 as rounded, with 2^19 to spare.  Every sub-sample of a pixel lies within 1/2 of its centre
// on either axis, so a pixel whose CENTRE lies outside the box grown by r + 1/2 + m has no covered sub-sample: that box of centres is
// what the cull, the bins (widened to whole pixels by floor and ceil) and the paint kernel's skip all use.  A disc is the segment
// of length zero: L = 0, t = 0, q = p exactly, so its own two-subtraction form below gives the same d2.
#include "model.h"
#include "data_layouts.h"
#include <cmath>

// the statement rounds every difference, product, quotient and sum: nothing may be contracted into fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int OT = DBM_OVERLAY_TILE;
constexpr int OV_THREADS = OT * OT;
constexpr int OV_CHUNK = DBM_OVERLAY_CHUNK;
constexpr int OV_MAX_BLOCKS = 4096;      // grid-stride launches over the primitives
constexpr int SCAN_ITEMS = 8;            // consecutive counts per lane of the scan kernels
constexpr int SCAN_TILE = OV_THREADS * SCAN_ITEMS;
constexpr int FULL_CHECK = 32;           // primitives between two looks at "is the whole wavefront covered"
typedef unsigned long long u64;
static_assert(OV_THREADS == 256 && OV_CHUNK == OV_THREADS && OV_CHUNK % FULL_CHECK == 0, "thread k stages primitive k");

struct Span {   // the closed box of pixel centres a primitive may touch
  double x0, x1, y0, y1;
};

inline int stride_blocks(long n) { return grid_stride_blocks(n, OV_THREADS, OV_MAX_BLOCKS); }

__device__ inline bool finite4(double a, double b, double c, double d) { return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d); }

// the box of the header comment; false: it holds no pixel centre of the image
__device__ inline bool centre_box(const OverlayLaunch& a, double ua, double va, double ub, double vb, Span* b) {
  const double M = fmax(fmax(fmax(fabs(ua), fabs(ub)), fmax(fabs(va), fabs(vb))), a.gmag);
  const double R = a.radius + 0.5 + (M * 0x1p-30 + 0x1p-480);
  b->x0 = fmin(ua, ub) - R;
  b->x1 = fmax(ua, ub) + R;
  b->y0 = fmin(va, vb) - R;
  b->y1 = fmax(va, vb) + R;
  return !(b->x1 < 0.0 || b->x0 > (double)(a.W - 1) || b->y1 < 0.0 || b->y0 > (double)(a.H - 1));
}

// the tiles [tx0, tx1] x [ty0, ty1] that hold a pixel centre of the box (which meets the image: centre_box said so)
__device__ inline void box_tiles(const OverlayLaunch& a, const Span& b, long* tx0, long* tx1, long* ty0, long* ty1) {
  const double c0 = floor(b.x0), c1 = ceil(b.x1), r0 = floor(b.y0), r1 = ceil(b.y1);
  *tx0 = (c0 > 0.0 ? (long)c0 : 0) / OT;                             // (c0 <= W - 1 and c1 >= 0 here, so the casts are in range)
  *tx1 = (c1 < (double)(a.W - 1) ? (long)c1 : a.W - 1) / OT;
  *ty0 = (r0 > 0.0 ? (long)r0 : 0) / OT;
  *ty1 = (r1 < (double)(a.H - 1) ? (long)r1 : a.H - 1) / OT;
}

// totals: [0] kept primitives, [1] entries the tile bins would hold, [2] primitives with a non-finite coordinate
template <int KIND>
__global__ __launch_bounds__(OV_THREADS) void overlay_cull_kernel(OverlayLaunch a) {
  const long stride = (long)gridDim.x * OV_THREADS;
  u64 bins = 0ull;
  for (long i0 = (long)blockIdx.x * OV_THREADS; i0 < a.n; i0 += stride) {   // (uniform per workgroup: the ballots need whole wavefronts)
    const long i = i0 + threadIdx.x;
    bool keep = false;
    double ua = 0.0, va = 0.0, ub = 0.0, vb = 0.0;
    if (i < a.n) {
      const double* p = a.prims + (long)a.stride * i;
      const double xa = p[0], ya = p[1], xb = KIND == DBM_OVERLAY_SEGMENTS ? p[2] : xa, yb = KIND == DBM_OVERLAY_SEGMENTS ? p[3] : ya;
      if (!finite4(xa, ya, xb, yb)) {
        atomicAdd(&a.totals[2], 1ull);
      } else {
        ua = (xa - a.x0) / a.dx;
        va = (ya - a.y0) / a.dy;
        ub = (xb - a.x0) / a.dx;
        vb = (yb - a.y0) / a.dy;
        Span b;
        if (finite4(ua, va, ub, vb) && centre_box(a, ua, va, ub, vb, &b)) {
          long tx0, tx1, ty0, ty1;
          box_tiles(a, b, &tx0, &tx1, &ty0, &ty1);
          keep = true;
          bins += (u64)(tx1 - tx0 + 1) * (u64)(ty1 - ty0 + 1);
        }
      }
    }
    const u64 at = wave_append(keep, &a.totals[0]);
    if (keep) {
      if (KIND == DBM_OVERLAY_SEGMENTS) {
        ((double2*)a.conv)[2 * at] = make_double2(ua, va);
        ((double2*)a.conv)[2 * at + 1] = make_double2(ub, vb);
      } else {
        ((double2*)a.conv)[at] = make_double2(ua, va);
      }
    }
  }
  if (bins) atomicAdd(&a.totals[1], bins);
}

// f(tile) for every tile of kept primitive j, as the cull pass counted them
template <int KIND, class F>
__device__ inline void kept_tiles(const OverlayLaunch& a, long j, F f) {
  const double2* src = (const double2*)a.conv;
  const double2 pa = KIND == DBM_OVERLAY_SEGMENTS ? src[2 * j] : src[j], pb = KIND == DBM_OVERLAY_SEGMENTS ? src[2 * j + 1] : pa;
  Span b;
  if (!centre_box(a, pa.x, pa.y, pb.x, pb.y, &b)) return;
  long tx0, tx1, ty0, ty1;
  box_tiles(a, b, &tx0, &tx1, &ty0, &ty1);
  for (long ty = ty0; ty <= ty1; ++ty)
    for (long tx = tx0; tx <= tx1; ++tx) f(ty * a.tiles_x + tx);
}

template <int KIND>
__global__ __launch_bounds__(OV_THREADS) void overlay_count_kernel(OverlayLaunch a) {
  const long stride = (long)gridDim.x * OV_THREADS;
  for (long j = (long)blockIdx.x * OV_THREADS + threadIdx.x; j < (long)a.kept; j += stride)
    kept_tiles<KIND>(a, j, [&](long t) { atomicAdd(&a.cnt[t], 1u); });
}

template <int KIND>
__global__ __launch_bounds__(OV_THREADS) void overlay_fill_kernel(OverlayLaunch a) {
  const long stride = (long)gridDim.x * OV_THREADS;
  for (long j = (long)blockIdx.x * OV_THREADS + threadIdx.x; j < (long)a.kept; j += stride)
    kept_tiles<KIND>(a, j, [&](long t) { a.entries[atomicAdd(&a.cursor[t], 1u)] = (unsigned)j; });
}

// ---- exclusive scan of cnt[0 .. nbins) into off (and cursor), off[nbins] = the sum ----
__device__ inline unsigned tile_counts(const OverlayLaunch& a, unsigned* k) {
  return scan_tile_items<OV_THREADS, SCAN_ITEMS, unsigned>(a.cnt, a.nbins, k, [](unsigned c) { return c; });
}

__global__ __launch_bounds__(OV_THREADS) void overlay_scan_sums_kernel(OverlayLaunch a) {
  unsigned k[SCAN_ITEMS], tot;
  block_exscan<OV_THREADS>(tile_counts(a, k), &tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(OV_THREADS) void overlay_scan_parts_kernel(OverlayLaunch a, long tiles) {
  const unsigned sum = scan_parts<OV_THREADS>(a.part, tiles);
  if (threadIdx.x == 0) a.off[a.nbins] = sum;
}

__global__ __launch_bounds__(OV_THREADS) void overlay_scan_offsets_kernel(OverlayLaunch a) {
  const long first = scan_tile_first<OV_THREADS, SCAN_ITEMS>();
  unsigned k[SCAN_ITEMS], tot;
  unsigned ex = block_exscan<OV_THREADS>(tile_counts(a, k), &tot) + a.part[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    if (first + j < a.nbins) {
      a.off[first + j] = ex;
      a.cursor[first + j] = ex;
    }
    ex += k[j];
  }
}

// ---- paint ----
// the offset of sub-sample j of S from the pixel's centre: (j + 1/2) / S - 1/2, exact
template <int S>
__device__ __forceinline__ constexpr double sub_offset(int j) { return ((double)j + 0.5) / (double)S - 0.5; }

template <int KIND, int S>
__global__ __launch_bounds__(OV_THREADS) void overlay_paint_kernel(OverlayLaunch a) {
  constexpr int ROW = KIND == DBM_OVERLAY_SEGMENTS ? 2 : 1;   // 16-byte pieces per primitive
  constexpr unsigned FULL = (1u << (S * S)) - 1u;
  constexpr unsigned D = (unsigned)(S * S) * 255u;
  __shared__ double2 sh[ROW * OV_CHUNK];
  __shared__ Span box[OV_CHUNK];
  const long tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const long r = ty * OT + (threadIdx.x >> 4), c = tx * OT + (threadIdx.x & 15);
  const bool valid = r < a.H && c < a.W;
  const double cu = (double)c, cv = (double)r;

  const unsigned* list = nullptr;
  long begin = 0, end = a.kept;
  if (a.entries) {
    list = a.entries;
    begin = a.off[tile];
    end = a.off[tile + 1];
  }

  unsigned mask = valid ? 0u : FULL;   // (a lane outside the image never holds its wavefront back)
  bool wave_done = __all(mask == FULL);
  for (long base = begin; base < end; base += OV_CHUNK) {
    const int n = (int)(end - base < OV_CHUNK ? end - base : OV_CHUNK);
    if ((int)threadIdx.x < n) {
      const long j = list ? (long)list[base + threadIdx.x] : base + threadIdx.x;
      const double2* src = (const double2*)a.conv + ROW * j;
      const double2 pa = src[0], pb = ROW == 2 ? src[ROW - 1] : pa;
      sh[ROW * threadIdx.x] = pa;
      if (ROW == 2) sh[ROW * threadIdx.x + ROW - 1] = pb;
      Span b;
      centre_box(a, pa.x, pa.y, pb.x, pb.y, &b);
      box[threadIdx.x] = b;
    }
    __syncthreads();
    for (int k0 = 0; k0 < n && !wave_done; k0 += FULL_CHECK) {
      const int k1 = k0 + FULL_CHECK < n ? k0 + FULL_CHECK : n;
      for (int k = k0; k < k1; ++k) {
        const Span b = box[k];
        if (mask == FULL || cu < b.x0 || cu > b.x1 || cv < b.y0 || cv > b.y1) continue;
        const double2 pa = sh[ROW * k];
        if (KIND == DBM_OVERLAY_SEGMENTS) {
          const double2 pb = sh[ROW * k + ROW - 1];
          const double ex = pb.x - pa.x, ey = pb.y - pa.y, L = ex * ex + ey * ey;
#pragma unroll
          for (int i = 0; i < S; ++i) {
            const double py = (cv + sub_offset<S>(i)) - pa.y;
#pragma unroll
            for (int j = 0; j < S; ++j) {
              const double px = (cu + sub_offset<S>(j)) - pa.x;
              double t = L > 0.0 ? (px * ex + py * ey) / L : 0.0;
              t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
              const double qx = px - t * ex, qy = py - t * ey, d2 = qx * qx + qy * qy;
              if (d2 <= a.r2) mask |= 1u << (i * S + j);
            }
          }
        } else {
#pragma unroll
          for (int i = 0; i < S; ++i) {
            const double py = (cv + sub_offset<S>(i)) - pa.y;
#pragma unroll
            for (int j = 0; j < S; ++j) {
              const double px = (cu + sub_offset<S>(j)) - pa.x;
              const double d2 = px * px + py * py;
              if (d2 <= a.r2) mask |= 1u << (i * S + j);
            }
          }
        }
      }
      wave_done = __all(mask == FULL);
    }
    if (__syncthreads_or(!wave_done) == 0) break;   // (also: the chunk is free for the next staging)
  }
  if (!valid || mask == 0u) return;

  // w src + (D - w) dst + D / 2 <= 255 D + D / 2 < 2^21: 32-bit integers
  const unsigned w = (unsigned)__popc(mask) * a.rgba[3];
  const long at = (r * a.W + c) * (long)a.channels;
  unsigned char* px = a.image + at;
  if (a.channels == 4 && a.word_aligned) {
    const unsigned old = *(const unsigned*)px;
    unsigned out = 0u;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const unsigned src = ch < 3 ? a.rgba[ch] : 255u, dst = (old >> (8 * ch)) & 255u;
      out |= ((w * src + (D - w) * dst + D / 2) / D) << (8 * ch);
    }
    *(unsigned*)px = out;
  } else {
    for (int ch = 0; ch < a.channels; ++ch) {
      const unsigned src = ch < 3 ? a.rgba[ch] : 255u, dst = px[ch];
      px[ch] = (unsigned char)((w * src + (D - w) * dst + D / 2) / D);
    }
  }
}

inline long scan_tiles(long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

template <int KIND>
void paint(const OverlayLaunch& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y)), block(OV_THREADS);
  if (a.S == 1) hipLaunchKernelGGL((overlay_paint_kernel<KIND, 1>), grid, block, 0, s, a);
  else if (a.S == 2) hipLaunchKernelGGL((overlay_paint_kernel<KIND, 2>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((overlay_paint_kernel<KIND, 4>), grid, block, 0, s, a);
}

}  // namespace

void overlay_geometry(OverlayLaunch& a) {
  a.tiles_x = (a.W + OT - 1) / OT;
  a.tiles_y = (a.H + OT - 1) / OT;
  a.nbins = a.tiles_x * a.tiles_y;
  a.radius = a.size * 0.5;          // exact
  a.r2 = a.radius * a.radius;       // one product, rounded: this translation unit is compiled with contraction off
  a.gmag = std::fmax(std::fmax((double)a.W, (double)a.H), a.radius);
}

// the one layout of the workspace; *staged = room for a host table of n rows of `stride` doubles if asked for, else null
size_t overlay_layout(OverlayLaunch& a, bool stage_prims_too, double** staged, Carver c) {
  a.totals = c.take<u64>(8);
  a.conv = c.take<double>((size_t)a.n * (a.kind == DBM_OVERLAY_SEGMENTS ? 4 : 2));
  a.cnt = c.take<unsigned>((size_t)a.nbins);
  a.cursor = c.take<unsigned>((size_t)a.nbins);
  a.off = c.take<unsigned>((size_t)(a.nbins + 1));
  a.part = c.take<unsigned>((size_t)scan_tiles(a.nbins));
  *staged = stage_prims_too ? c.take<double>((size_t)a.n * (size_t)a.stride) : nullptr;
  return c.bytes();
}

size_t overlay_workspace(const OverlayLaunch& a, bool stage_prims_too) { OverlayLaunch b = a; double* p; return overlay_layout(b, stage_prims_too, &p, Carver(nullptr)); }

double* overlay_carve(OverlayLaunch& a, void* ws, bool stage_prims_too) { double* p; overlay_layout(a, stage_prims_too, &p, Carver(ws)); return p; }

void launch_overlay_cull(const OverlayLaunch& a, hipStream_t s) {
  DBM_HIP(hipMemsetAsync(a.totals, 0, sizeof(u64) * 8, s));
  if (a.n > 0) {
    if (a.kind == DBM_OVERLAY_SEGMENTS) hipLaunchKernelGGL(overlay_cull_kernel<DBM_OVERLAY_SEGMENTS>, dim3(stride_blocks(a.n)), dim3(OV_THREADS), 0, s, a);
    else hipLaunchKernelGGL(overlay_cull_kernel<DBM_OVERLAY_DISCS>, dim3(stride_blocks(a.n)), dim3(OV_THREADS), 0, s, a);
  }
  DBM_HIP(hipGetLastError());
}

void launch_overlay_bin(const OverlayLaunch& a, hipStream_t s) {
  const long tiles = scan_tiles(a.nbins);
  const dim3 over_kept(stride_blocks((long)a.kept)), block(OV_THREADS);
  const bool seg = a.kind == DBM_OVERLAY_SEGMENTS;
  DBM_HIP(hipMemsetAsync(a.cnt, 0, 4 * (size_t)a.nbins, s));
  if (seg) hipLaunchKernelGGL(overlay_count_kernel<DBM_OVERLAY_SEGMENTS>, over_kept, block, 0, s, a);
  else hipLaunchKernelGGL(overlay_count_kernel<DBM_OVERLAY_DISCS>, over_kept, block, 0, s, a);
  hipLaunchKernelGGL(overlay_scan_sums_kernel, dim3((unsigned)tiles), block, 0, s, a);
  hipLaunchKernelGGL(overlay_scan_parts_kernel, dim3(1), block, 0, s, a, tiles);
  hipLaunchKernelGGL(overlay_scan_offsets_kernel, dim3((unsigned)tiles), block, 0, s, a);
  if (seg) hipLaunchKernelGGL(overlay_fill_kernel<DBM_OVERLAY_SEGMENTS>, over_kept, block, 0, s, a);
  else hipLaunchKernelGGL(overlay_fill_kernel<DBM_OVERLAY_DISCS>, over_kept, block, 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_overlay_paint(const OverlayLaunch& a, hipStream_t s) {
  if (a.kind == DBM_OVERLAY_SEGMENTS) paint<DBM_OVERLAY_SEGMENTS>(a, s);
  else paint<DBM_OVERLAY_DISCS>(a, s);
  DBM_HIP(hipGetLastError());
}
