// Grid sampling along survey tracks (reference srgan_train.py:1458-1464 and deepbedmap.py:530-574: `gmt.grdtrack(points, grid)`
// followed by the RMSE of z_interpolated - z).  One lane per point: the float32 grid is evaluated at (x, y) with GMT's nearest,
// bilinear or bicubic (Keys, a = -1/2) interpolant in float64, and the finite along-track errors are reduced to
// (count, mean, M2, sum e^2, min, max) -- lane partials merged with Chan's pairwise update in a fixed tree (lanes, waves through
// LDS), one partial per workgroup, folded in workgroup order by one finishing workgroup.  The launch geometry depends on n only,
// so the statistics are the same bits from call to call.  Semantics (DESIGN.md "Track sampling"):
//   - node (r, c) at (x0 + c dx, y0 + r dy); t = (x - x0) / dx, s = (y - y0) / dy; the domain is [0, W-1] x [0, H-1] (gridline)
//     or [-1/2, W-1/2] x [-1/2, H-1/2] (pixel); outside it, or NaN coordinates: NaN;
//   - ghost nodes (up to two beyond every edge): linear extrapolation z[-k] = z[0] + k (z[0] - z[1]), columns first, then rows;
//   - NaN nodes: with V the non-NaN stencil nodes and wsum their weight sum, the result is sum_V w z / wsum if wsum + 1e-9 >= threshold,
//     else NaN (no division when every node is valid).
#include "model.h"
#include "data_prims.h"
#include <cmath>

namespace {

constexpr int TRACK_THREADS = 256;
constexpr int TRACK_MAX_BLOCKS = 1024;  // 4 workgroups per CU, all resident at once (bicubic: 91 VGPRs, 5 waves per SIMD)

struct Moments {  // one partial of the error statistics
  double n, mean, m2, ss, mn, mx;
};

__device__ inline Moments moments_empty() { return {0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

__device__ inline void moments_add(Moments& a, double e) {  // Welford
  a.n += 1.0;
  const double d = e - a.mean;
  a.mean += d / a.n;
  a.m2 += d * (e - a.mean);
  a.ss += e * e;
  a.mn = fmin(a.mn, e);
  a.mx = fmax(a.mx, e);
}

__device__ inline Moments moments_merge(const Moments& a, const Moments& b) {  // Chan et al.
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Moments r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
  r.ss = a.ss + b.ss;
  r.mn = fmin(a.mn, b.mn);
  r.mx = fmax(a.mx, b.mx);
  return r;
}

// value of the (possibly ghost) node (rr, cc), rr in [-2, H+1], cc in [-2, W+1]; H, W >= 2
__device__ inline double row_node(const float* __restrict__ g, long W, long r, long cc) {
  const float* row = g + r * W;
  if (cc < 0) {
    const double a = row[0], b = row[1];
    return a + (double)(-cc) * (a - b);
  }
  if (cc > W - 1) {
    const double a = row[W - 1], b = row[W - 2];
    return a + (double)(cc - (W - 1)) * (a - b);
  }
  return row[cc];
}
__device__ inline double ghost_node(const float* __restrict__ g, long H, long W, long rr, long cc) {
  if (rr < 0) {
    const double a = row_node(g, W, 0, cc), b = row_node(g, W, 1, cc);
    return a + (double)(-rr) * (a - b);
  }
  if (rr > H - 1) {
    const double a = row_node(g, W, H - 1, cc), b = row_node(g, W, H - 2, cc);
    return a + (double)(rr - (H - 1)) * (a - b);
  }
  return row_node(g, W, rr, cc);
}

template <int K>
__device__ inline void stencil_weights(double u, double* w) {
  if (K == 2) {
    w[0] = 1.0 - u;
    w[1] = u;
  } else {  // Keys cubic convolution, a = -1/2
    w[0] = u * (u * (-0.5 * u + 1.0) - 0.5);
    w[1] = u * u * (1.5 * u - 2.5) + 1.0;
    w[2] = u * (u * (-1.5 * u + 2.0) + 0.5);
    w[3] = u * u * (0.5 * u - 0.5);
  }
}

// INTERP: 0 nearest, 1 bilinear, 2 bicubic
template <int INTERP>
__device__ double sample(const TrackLaunch& a, double x, double y) {
  const double t = (x - a.x0) / a.dx, s = (y - a.y0) / a.dy;
  if (!(t >= a.tlo && t <= a.thi && s >= a.slo && s <= a.shi)) return __builtin_nan("");  // (NaN coordinates fail too)
  if (INTERP == 0) {
    long r = (long)floor(s + 0.5), c = (long)floor(t + 0.5);
    r = r < 0 ? 0 : (r > a.H - 1 ? a.H - 1 : r);
    c = c < 0 ? 0 : (c > a.W - 1 ? a.W - 1 : c);
    return (double)a.grid[r * a.W + c];
  }
  constexpr int K = INTERP == 1 ? 2 : 4;
  const double cf = floor(t), rf = floor(s);
  double wc[K], wr[K];
  stencil_weights<K>(t - cf, wc);
  stencil_weights<K>(s - rf, wr);
  const long c0 = (long)cf - (K == 4 ? 1 : 0), r0 = (long)rf - (K == 4 ? 1 : 0);
  double acc = 0.0, wsum = 0.0;
  bool holes = false;
  if (r0 >= 0 && r0 + K - 1 <= a.H - 1 && c0 >= 0 && c0 + K - 1 <= a.W - 1) {  // the stencil lies inside the grid
    const float* p = a.grid + r0 * a.W + c0;
    float v[K][K];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int i = 0; i < K; ++i) v[j][i] = p[j * a.W + i];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double w = wr[j] * wc[i], z = v[j][i];
        if (z == z) { acc += w * z; wsum += w; } else holes = true;
      }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double w = wr[j] * wc[i], z = ghost_node(a.grid, a.H, a.W, r0 + j, c0 + i);
        if (z == z) { acc += w * z; wsum += w; } else holes = true;
      }
  }
  if (!holes) return acc;
  return wsum + 1e-9 >= a.threshold ? acc / wsum : __builtin_nan("");
}

template <int INTERP>
__global__ __launch_bounds__(TRACK_THREADS) void grid_track_kernel(TrackLaunch a) {
  Moments m = moments_empty();
  const long stride = (long)gridDim.x * TRACK_THREADS;
  for (long i = (long)blockIdx.x * TRACK_THREADS + threadIdx.x; i < a.n; i += stride) {
    const double* p = a.points + i * a.ncol;
    const double zi = sample<INTERP>(a, p[0], p[1]);
    if (a.z_out) a.z_out[i] = zi;
    if (a.part) {
      const double e = zi - p[2];
      if (isfinite(e)) moments_add(m, e);
    }
  }
  if (!a.part) return;
  m = block_reduce<TRACK_THREADS>(m, moments_merge);
  if (threadIdx.x == 0) {
    double* o = a.part + 6 * (long)blockIdx.x;
    o[0] = m.n; o[1] = m.mean; o[2] = m.m2; o[3] = m.ss; o[4] = m.mn; o[5] = m.mx;
  }
}

// one workgroup folds the partials in order (fold_partials); stats = count, mean, std (ddof 1), min, max, rmse
__global__ __launch_bounds__(TRACK_THREADS) void grid_track_finish_kernel(const double* __restrict__ part, int blocks, double* stats) {
  const Moments m = fold_partials<TRACK_THREADS>(blocks, moments_empty(), [part](long b) {
    const double* q = part + 6 * b;
    return Moments{q[0], q[1], q[2], q[3], q[4], q[5]};
  }, moments_merge);
  if (threadIdx.x != 0) return;
  const double nan = __builtin_nan("");
  stats[0] = m.n;
  stats[1] = m.n > 0.0 ? m.mean : nan;
  stats[2] = m.n > 1.0 ? sqrt(m.m2 / (m.n - 1.0)) : nan;
  stats[3] = m.n > 0.0 ? m.mn : nan;
  stats[4] = m.n > 0.0 ? m.mx : nan;
  stats[5] = m.n > 0.0 ? sqrt(m.ss / m.n) : nan;
}

// `grdsample -T`: one lane per cell centre of the unit-geometry gridline grid
__global__ __launch_bounds__(TRACK_THREADS) void grid_to_pixel_kernel(TrackLaunch a, float* __restrict__ out) {
  const long wo = a.W - 1, stride = (long)gridDim.x * TRACK_THREADS;
  for (long i = (long)blockIdx.x * TRACK_THREADS + threadIdx.x; i < a.n; i += stride) {
    const long r = i / wo, c = i - r * wo;
    out[i] = (float)sample<2>(a, (double)c + 0.5, (double)r + 0.5);
  }
}

}  // namespace

int grid_track_blocks(long n) { return grid_stride_blocks(n, TRACK_THREADS, TRACK_MAX_BLOCKS); }

void launch_grid_track(const TrackLaunch& a, double* stats, hipStream_t s) {
  const int blocks = grid_track_blocks(a.n);
  if (a.n > 0 && (a.z_out || a.part)) {
    switch (a.interp) {
      case 0: hipLaunchKernelGGL(grid_track_kernel<0>, dim3(blocks), dim3(TRACK_THREADS), 0, s, a); break;
      case 1: hipLaunchKernelGGL(grid_track_kernel<1>, dim3(blocks), dim3(TRACK_THREADS), 0, s, a); break;
      default: hipLaunchKernelGGL(grid_track_kernel<2>, dim3(blocks), dim3(TRACK_THREADS), 0, s, a); break;
    }
    DBM_HIP(hipGetLastError());
  }
  if (a.part) {
    // n == 0: nothing was launched above, the fold reads no partial and writes count 0 and NaN
    hipLaunchKernelGGL(grid_track_finish_kernel, dim3(1), dim3(TRACK_THREADS), 0, s, a.part, a.n > 0 ? blocks : 0, stats);
    DBM_HIP(hipGetLastError());
  }
}

void launch_grid_to_pixel(const float* in, long H, long W, double threshold, float* out, hipStream_t s) {
  TrackLaunch a;
  a.grid = in;
  a.H = H; a.W = W;
  a.x0 = 0.0; a.y0 = 0.0; a.dx = 1.0; a.dy = 1.0;
  a.tlo = 0.0; a.thi = (double)(W - 1);
  a.slo = 0.0; a.shi = (double)(H - 1);
  a.points = nullptr;
  a.n = (H - 1) * (W - 1);
  a.ncol = 2;
  a.interp = 2;
  a.threshold = threshold;
  a.z_out = nullptr;
  a.part = nullptr;
  hipLaunchKernelGGL(grid_to_pixel_kernel, dim3(grid_track_blocks(a.n)), dim3(TRACK_THREADS), 0, s, a, out);
  DBM_HIP(hipGetLastError());
}
