// Colour relief and hillshade of a resident plane (dbm_grid_relief, dbm_grid_shade_stats; the colour tables, the PNG container and the
// public calls are deepbedmap_amd/relief.py).  Reference: deepbedmap.py:758-775 ("Show *the* DeepBedMap": gmt.makecpt(cmap="oleron",
// series=[-4500, 4500]) and fig.grdimage(..., cmap=True, Q=True)) and paper_figures.py:692-699 (the same with shading="+d").  The rules
// below are this project's own -- GMT's HSV illumination, its per-version hinge handling and its dpi resampling are not restated --
// and are stated once more, with the reasons, in DESIGN.md 6n.
//
// Table.  n slices; edges E_0 < ... < E_n (float64); slice i has the colours c0_i, c1_i (three bytes each) at its two ends; B, F, N are
// the colours below E_0, above E_n and of NaN.
//
// Pixel (z the float32 sample, v = (double)z; every operation below is ONE IEEE float64 operation, never an FMA):
//   colour   NaN: N (alpha 0 where there are four channels; alpha is 255 everywhere else), and the pixel is not shaded.
//            v < E_0: B.  v > E_n: F (so -inf is B and +inf is F).
//            else i = the largest index <= n - 1 with E_i <= v, t = (v - E_i) / (E_{i+1} - E_i), and per channel
//            u = c0 + (c1 - c0) * t: the product rounded, then the sum rounded.
//   shade    I = k * atan((g - mean) / sigma) where g is defined, else 0.  I >= 0: u' = u + (255 - u) * I.  I < 0: u' = u + u * I.
//   byte     floor(u' + 0.5), clamped to 0 .. 255.
// Gradient g at (r, c), rows north-up, index units:
//   dx = (z[r, c + 1] - z[r, c - 1]) * 0.5; at the first column (z[r, 1] - z[r, 0]) * 1, at the last (z[r, W - 1] - z[r, W - 2]) * 1;
//   dy = (z[r - 1, c] - z[r + 1, c]) * 0.5 (northward); at the first row (z[0, c] - z[1, c]) * 1, at the last (z[H - 2, c] - z[H - 1, c]) * 1;
//   g = -(dx * sin_a + (dy * aspect) * cos_a);
//   defined only where the four samples it reads are finite; nowhere if W == 1 or H == 1.
// Statistics (dbm_grid_shade_stats): n = the number of defined g, mean = sum g / n, sigma = sqrt(sum (g - mean)^2 / (n - 1)): two
// passes, float64, in the fixed order of data_prims.h's reduction over a grid that depends on H * W alone.
//
// Decomposition.  A workgroup of 256 threads walks tiles of 16 rows x 64 columns in grid-stride order.  It stages the table ONCE in
// LDS (8 (n + 1) bytes of edges, 6 n bytes of colours: 28 680 bytes at n = 2048, sized per call), then per tile the samples with their
// one-pixel halo (18 x 66 floats, rows read coalesced; row stride 69 floats: 69 = 5 (mod 64), so the four rows a wave reads at a
// column stride of four floats fall on different banks).  Thread (t / 16, t % 16) owns four consecutive pixels of one row: 16 bytes in,
// 12 or 16 bytes out, one 16-byte store per lane with four channels.  The slice search is a branch-free binary search over the edges
// in LDS: ceil(log2 n) steps, the same number in every lane.  The unshaded variant reads no neighbours: it has no tile and no barrier
// per tile, and loads its four samples with one 16-byte load per lane.
#include "kernels.h"
#include "data_prims.h"

namespace {

constexpr int RELIEF_THREADS = 256;
constexpr int RELIEF_TW = 64, RELIEF_TH = 16;
constexpr int RELIEF_STRIDE = 69;
constexpr int RELIEF_MAX_GROUPS = 2048;

typedef uint32_t relief_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t relief_u32x3 __attribute__((ext_vector_type(3), aligned(4)));
typedef float relief_f32x4 __attribute__((ext_vector_type(4), aligned(4)));

// The gradient of the header; z(r, c) returns the float32 sample.  False where g is not defined.
template <class Sample>
__device__ __forceinline__ bool relief_gradient(Sample z, long H, long W, long r, long c, double sin_a, double cos_a, double aspect, double& g) {
#pragma clang fp contract(off)
  if (H < 2 || W < 2) return false;
  const long cl = c > 0 ? c - 1 : c, cr = c < W - 1 ? c + 1 : c;
  const long ru = r > 0 ? r - 1 : r, rd = r < H - 1 ? r + 1 : r;
  const float zl = z(r, cl), zr = z(r, cr), zu = z(ru, c), zd = z(rd, c);
  if (!(isfinite(zl) && isfinite(zr) && isfinite(zu) && isfinite(zd))) return false;
  const double dx = ((double)zr - (double)zl) * (cr - cl == 2 ? 0.5 : 1.0);
  const double dy = ((double)zu - (double)zd) * (rd - ru == 2 ? 0.5 : 1.0);
  const double px = dx * sin_a;
  const double py = (dy * aspect) * cos_a;
  g = -(px + py);
  return true;
}

// Four pixels of one thread at once: the three colour bytes of each, packed little endian with the alpha above them.  Branch-free: the
// slice search and the interpolation run for every pixel -- the four searches advance together, so their LDS reads overlap -- and B, F
// and N replace the result afterwards; what an out-of-table or NaN sample computes on the way (infinities, NaN) is never kept.
template <bool SHADE>
__device__ __forceinline__ void relief_pixels(const float (&z)[4], const bool (&has_g)[4], const double (&g)[4], const double* edges,
                                              const uint8_t* cols, const ReliefLaunch& a, int top, uint32_t (&px)[4]) {
#pragma clang fp contract(off)
  const int n = a.n_slices;
  double v[4];
  int i[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = (double)z[q];
    i[q] = 0;
  }
  for (int step = top; step > 0; step >>= 1) {   // the answer lies in [i, i + 2 step): a candidate beyond n - 1 is n - 1
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = i[q] + step < n - 1 ? i[q] + step : n - 1;
      i[q] = edges[j] <= v[q] ? j : i[q];
    }
  }
  const double lo = edges[0], hi = edges[n];
  const uint32_t nan_px = (uint32_t)a.bfn[6] | ((uint32_t)a.bfn[7] << 8) | ((uint32_t)a.bfn[8] << 16);   // N: alpha 0, never shaded
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double e0 = edges[i[q]];
    const double t = (v[q] - e0) / (edges[i[q] + 1] - e0);
    const bool below = v[q] < lo, above = v[q] > hi;
    double I = 0.0;
    if (SHADE) I = has_g[q] ? a.k * atan((g[q] - a.mean) / a.sigma) : 0.0;
    uint32_t p = 0xFF000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double c0 = (double)cols[6 * i[q] + ch], c1 = (double)cols[6 * i[q] + 3 + ch];
      const double product = (c1 - c0) * t;
      double u = c0 + product;
      u = below ? (double)a.bfn[ch] : (above ? (double)a.bfn[3 + ch] : u);
      if (SHADE) {   // (I = 0 leaves u as it is: (255 - u) * 0 = +0 for u <= 255)
        const double shade = I >= 0.0 ? (255.0 - u) * I : u * I;
        u = u + shade;
      }
      const double w = floor(u + 0.5);
      p |= (uint32_t)(w < 0.0 ? 0.0 : (w > 255.0 ? 255.0 : w)) << (8 * ch);
    }
    px[q] = z[q] != z[q] ? nan_px : p;
  }
}

template <bool SHADE>
__global__ __launch_bounds__(RELIEF_THREADS) void grid_relief_kernel(ReliefLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char relief_lds[];
  const int n = a.n_slices;
  double* edges = (double*)relief_lds;                                   // n + 1
  float* tile = (float*)(edges + n + 1);                                 // shaded: (TH + 2) x STRIDE
  uint8_t* cols = (uint8_t*)(tile + (SHADE ? (RELIEF_TH + 2) * RELIEF_STRIDE : 0));   // 6 n
  for (int k = threadIdx.x; k <= n; k += RELIEF_THREADS) edges[k] = a.edges[k];
  for (int k = threadIdx.x; k < 6 * n; k += RELIEF_THREADS) cols[k] = a.colors[k];
  int top = 1;
  while (2 * top <= n - 1) top *= 2;
  constexpr int LW = RELIEF_TW + 2, LH = RELIEF_TH + 2;
  const int H = (int)a.H, W = (int)a.W;   // (H, W and H * W are below 2^31)
  const int tiles_x = (W + RELIEF_TW - 1) / RELIEF_TW, tiles_y = (H + RELIEF_TH - 1) / RELIEF_TH;
  const int ly = threadIdx.x / 16, lx = threadIdx.x % 16;
  if (!SHADE) __syncthreads();   // the table is staged (the shaded variant's loop opens with a barrier)
  for (long tl = blockIdx.x; tl < (long)tiles_x * tiles_y; tl += gridDim.x) {
    const int r0 = (int)(tl / tiles_x) * RELIEF_TH, c0 = (int)(tl % tiles_x) * RELIEF_TW;
    if (SHADE) {
      __syncthreads();   // the table is staged; the previous tile has been read
      for (int e = threadIdx.x; e < LW * LH; e += RELIEF_THREADS) {
        const int r = r0 - 1 + e / LW, c = c0 - 1 + e % LW;
        tile[(e / LW) * RELIEF_STRIDE + e % LW] = r >= 0 && r < H && c >= 0 && c < W ? a.plane[(long)r * W + c] : __builtin_nanf("");
      }
      __syncthreads();
    }
    const int r = r0 + ly, c = c0 + 4 * lx;
    if (r >= H || c >= W) continue;   // (no barrier below this line inside the iteration)
    const long at = (long)r * W + c;   // below 2^31
    float z[4];
    bool has_g[4];
    double g[4];
    if (SHADE) {
      auto sample = [&](long rr, long cc) { return tile[(rr - r0 + 1) * RELIEF_STRIDE + (cc - c0 + 1)]; };
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        z[q] = sample(r, c + q);   // (NaN beyond the plane: computed, never stored)
        g[q] = 0.0;
        has_g[q] = c + q < W && relief_gradient(sample, a.H, a.W, r, c + q, a.sin_a, a.cos_a, a.aspect, g[q]);
      }
    } else {   // no neighbours needed: the samples come straight from memory, sixteen bytes per lane
      if (c + 4 <= W) {
        const relief_f32x4 four = *(const relief_f32x4*)(a.plane + at);
        z[0] = four.x; z[1] = four.y; z[2] = four.z; z[3] = four.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = c + q < W ? a.plane[at + q] : __builtin_nanf("");
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g[q] = 0.0;
        has_g[q] = false;
      }
    }
    uint32_t px[4];
    relief_pixels<SHADE>(z, has_g, g, edges, cols, a, top, px);
    if (a.channels == 4) {
      if (c + 4 <= W) {
        *(relief_u32x4*)(a.out + 4 * at) = relief_u32x4{px[0], px[1], px[2], px[3]};
      } else {
        for (int q = 0; c + q < W; ++q) ((uint32_t*)a.out)[at + q] = px[q];
      }
    } else if (c + 4 <= W && (at & 3) == 0) {   // twelve bytes on a word boundary
      const uint32_t p0 = px[0] & 0xFFFFFFu, p1 = px[1] & 0xFFFFFFu, p2 = px[2] & 0xFFFFFFu, p3 = px[3] & 0xFFFFFFu;
      *(relief_u32x3*)(a.out + 3 * at) = relief_u32x3{p0 | (p1 << 24), (p1 >> 8) | (p2 << 16), (p2 >> 16) | (p3 << 8)};
    } else {
      for (int q = 0; q < 4 && c + q < W; ++q)
        for (int ch = 0; ch < 3; ++ch) a.out[3 * (at + q) + ch] = (uint8_t)(px[q] >> (8 * ch));
    }
  }
}

// ---- statistics of the gradient: two passes, each a grid of partial sums and one workgroup that folds them in order ----
struct ShadeSum {
  double s;
  long long n;
};
__device__ __forceinline__ ShadeSum shade_merge(const ShadeSum& a, const ShadeSum& b) { return ShadeSum{a.s + b.s, a.n + b.n}; }

// pass 0: part[g] = {sum g, count}; pass 1: part[g] = {sum (g - stats[1])^2, count}
__global__ __launch_bounds__(RELIEF_THREADS) void shade_partials_kernel(ReliefLaunch a, int pass, const double* stats, ShadeSum* part) {
#pragma clang fp contract(off)
  const double mean = pass ? stats[1] : 0.0;
  auto sample = [&](long rr, long cc) { return a.plane[rr * a.W + cc]; };
  ShadeSum v{0.0, 0};
  for (long p = (long)blockIdx.x * RELIEF_THREADS + threadIdx.x; p < a.H * a.W; p += (long)gridDim.x * RELIEF_THREADS) {
    double g;
    if (!relief_gradient(sample, a.H, a.W, p / a.W, p % a.W, a.sin_a, a.cos_a, a.aspect, g)) continue;
    const double d = g - mean;
    const double term = pass ? d * d : g;
    v.s = v.s + term;
    v.n += 1;
  }
  v = block_reduce<RELIEF_THREADS>(v, shade_merge);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// pass 0: stats = {n, sum / n (0 if n == 0), 0}; pass 1: stats[2] = sqrt(sum / (n - 1)) (0 if n < 2)
__global__ __launch_bounds__(RELIEF_THREADS) void shade_fold_kernel(const ShadeSum* part, int groups, int pass, double* stats) {
  const ShadeSum v = fold_partials<RELIEF_THREADS>((long)groups, ShadeSum{0.0, 0}, [&](long k) { return part[k]; }, shade_merge);
  if (threadIdx.x != 0) return;
  if (pass == 0) {
    stats[0] = (double)v.n;
    stats[1] = v.n > 0 ? v.s / (double)v.n : 0.0;
    stats[2] = 0.0;
  } else {
    stats[2] = v.n > 1 ? sqrt(v.s / (double)(v.n - 1)) : 0.0;
  }
}

}  // namespace

void launch_grid_relief(const ReliefLaunch& a, hipStream_t s) {
  const long tiles = ((a.W + RELIEF_TW - 1) / RELIEF_TW) * ((a.H + RELIEF_TH - 1) / RELIEF_TH);
  const unsigned groups = (unsigned)(tiles < RELIEF_MAX_GROUPS ? tiles : RELIEF_MAX_GROUPS);
  const size_t lds = 8 * ((size_t)a.n_slices + 1) + (a.shade ? 4 * (size_t)(RELIEF_TH + 2) * RELIEF_STRIDE : 0) + 6 * (size_t)a.n_slices;
  if (a.shade) hipLaunchKernelGGL(grid_relief_kernel<true>, dim3(groups), dim3(RELIEF_THREADS), lds, s, a);
  else hipLaunchKernelGGL(grid_relief_kernel<false>, dim3(groups), dim3(RELIEF_THREADS), lds, s, a);
  DBM_HIP(hipGetLastError());
}

namespace {
// the workspace of launch_shade_stats: the three results first, then one partial sum per workgroup
struct ShadeStatsLayout {
  double* stats;
  ShadeSum* part;
  int groups;
  ShadeStatsLayout(Carver& carve, long H, long W) {
    groups = grid_stride_blocks(H * W, RELIEF_THREADS, RELIEF_MAX_GROUPS);
    stats = carve.take<double>(3);
    part = carve.take<ShadeSum>((size_t)groups);
  }
};
}  // namespace

size_t shade_stats_workspace(long H, long W) {
  Carver measure(nullptr);
  ShadeStatsLayout layout(measure, H, W);
  return measure.bytes();
}

void launch_shade_stats(const ReliefLaunch& a, void* ws, hipStream_t s) {
  Carver carve(ws);
  const ShadeStatsLayout layout(carve, a.H, a.W);
  double* stats = layout.stats;
  ShadeSum* part = layout.part;
  const int groups = layout.groups;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(shade_partials_kernel, dim3((unsigned)groups), dim3(RELIEF_THREADS), 0, s, a, pass, stats, part);
    hipLaunchKernelGGL(shade_fold_kernel, dim3(1), dim3(RELIEF_THREADS), 0, s, part, groups, pass, stats);
  }
  DBM_HIP(hipGetLastError());
}
