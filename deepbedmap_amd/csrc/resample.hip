// The grids DeepBedMap is compared against (reference deepbedmap.py:323-331 the bicubic BEDMAP2 baseline, :348-356 the synthetic grid
// brought to 250 m, both `skimage.transform.rescale`; paper_figures.py:847-867 `standard_deviation_2d`, the roughness grids).  Whole-plane
// passes over grids resident in HBM, float64 arithmetic, 64-bit element offsets, launch geometry a function of the shapes only, no float
// atomics: the same bits from call to call.  Semantics (DESIGN.md "Comparison grids"):
//
// dbm_grid_rescale -- the scipy.ndimage chain behind current scikit-image's rescale:
//   minmax_kernel / minmax_finish_kernel   min and max of the (cast) input, for the clip; partials per workgroup, folded by one workgroup;
//   gauss_weights_kernel                   exp(-x^2 / (2 sigma^2)), x = -radius..radius, radius = int(4 sigma + 0.5), normalised;
//   gauss_kernel<AXIS>                     correlate1d with those weights over the mirrored signal (d c b | a b c d | c b a), one lane per
//                                          value, a workgroup = 256 columns of one row (the taps of a lane's neighbours share their lines);
//   prefilter_rows_kernel                  cubic B-spline prefilter along axis 0 (pole sqrt(3) - 2, gain 6): one lane per column, the rows cut
//                                          into chunks of PRE_ROWS; a lane warms the causal recursion up over the PRE_WARM rows before its
//                                          chunk (mirrored beyond row 0: the truncated mirror sum that starts scipy's recursion), runs it
//                                          PRE_WARM rows past the chunk while summing the anticausal start value forward, and closes with
//                                          scipy's end formula (exact at the last row, |pole|^PRE_WARM = 5e-19 off elsewhere);
//   prefilter_cols_kernel                  the same along axis 1: PRE_TILE_ROWS rows x (PRE_COLS + 2 PRE_WARM) columns staged in LDS with an
//                                          odd row stride (8-byte accesses of 32 lanes fall into 32 distinct bank pairs), one lane per row;
//   zoom_kernel<ORDER>                     one lane per output value: coordinate (o + 0.5) in / out - 0.5 folded into [0, n - 1] by scipy's
//                                          mirror rule, linear or cubic B-spline weights over mirrored node indices, clip, one rounding to
//                                          float32.
//   Every pass reads one plane and writes another (a chunk's warm-up rows belong to its neighbours), so two float64 planes alternate.
//
// dbm_grid_rolling_std -- one lane per node, a tile with its halo staged in LDS: count, sum and sum of squares of the window's valid nodes,
//   shifted by one of them (the centre node, else the first valid node in row-major order), so that nothing cancels and a constant window
//   gives exactly 0.
#include "model.h"
#include "data_prims.h"
#include <cmath>

namespace {

constexpr int RS_THREADS = 256;
constexpr int MM_BLOCKS = 1024;
constexpr int PRE_WARM = 32;        // |pole|^32 = 5e-19
constexpr int PRE_ROWS = 256;       // rows per chunk of the axis-0 prefilter
constexpr int PRE_COLS = 128;       // columns per chunk of the axis-1 prefilter
constexpr int PRE_TILE_ROWS = 32;   // rows per workgroup of the axis-1 prefilter
constexpr int PRE_SPAN = PRE_COLS + 2 * PRE_WARM;
constexpr int PRE_STRIDE = PRE_SPAN + 1;   // odd
constexpr int STD_TW = 64, STD_TH = 16;    // roughness: output tile of a workgroup

#define POLE (-0.26794919243112270647)     // sqrt(3) - 2

// a plane that is either the caller's float32 grid (optionally cast like `.astype(np.int32)`) or a float64 workspace plane
struct Src {
  const float* f;
  const double* d;
  int cast;
  __device__ inline double at(long i) const {
    if (d) return d[i];
    const float v = f[i];
    return cast ? (double)(int)v : (double)v;
  }
};

__device__ inline long mirror_index(long i, long n) {
  if (n == 1) return 0;
  const long p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// scipy's fold of a coordinate outside [0, n - 1] (NI_EXTEND_MIRROR)
__device__ inline double mirror_coordinate(double c, long n) {
  if (n <= 1) return 0.0;
  const double p = (double)(2 * n - 2);
  if (c < 0.0) {
    c = p * (double)(long)(-c / p) + c;
    return c <= (double)(1 - n) ? c + p : -c;
  }
  if (c > (double)(n - 1)) {
    c -= p * (double)(long)(c / p);
    return c >= (double)n ? p - c : c;
  }
  return c;
}

struct MinMax {
  double mn, mx;
};
__device__ inline MinMax minmax_merge(const MinMax& a, const MinMax& b) { return {fmin(a.mn, b.mn), fmax(a.mx, b.mx)}; }

__global__ __launch_bounds__(RS_THREADS) void minmax_kernel(Src src, long total, double* part) {
  MinMax m = {INFINITY, -INFINITY};
  const long stride = (long)gridDim.x * RS_THREADS;
  for (long i = (long)blockIdx.x * RS_THREADS + threadIdx.x; i < total; i += stride) {
    const double v = src.at(i);
    m.mn = fmin(m.mn, v);
    m.mx = fmax(m.mx, v);
  }
  m = block_reduce<RS_THREADS>(m, minmax_merge);
  if (threadIdx.x == 0) {
    part[2 * (long)blockIdx.x] = m.mn;
    part[2 * (long)blockIdx.x + 1] = m.mx;
  }
}

__global__ __launch_bounds__(RS_THREADS) void minmax_finish_kernel(const double* part, int blocks, double* out) {
  const MinMax m = fold_partials<RS_THREADS>(blocks, MinMax{INFINITY, -INFINITY}, [part](long b) { return MinMax{part[2 * b], part[2 * b + 1]}; },
                                             minmax_merge);
  if (threadIdx.x == 0) {
    out[0] = m.mn;
    out[1] = m.mx;
  }
}

// one workgroup: w[k] = exp(-0.5 / sigma^2 (k - radius)^2) / sum, the sum taken in index order by every thread alike
__global__ __launch_bounds__(RS_THREADS) void gauss_weights_kernel(double sigma, int radius, double* w) {
  const int n = 2 * radius + 1;
  const double s = -0.5 / (sigma * sigma);
  for (int k = threadIdx.x; k < n; k += RS_THREADS) {
    const double x = (double)(k - radius);
    w[k] = exp(s * (x * x));
  }
  __syncthreads();
  double sum = 0.0;
  for (int k = 0; k < n; ++k) sum += w[k];
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += RS_THREADS) w[k] = w[k] / sum;
}

template <int AXIS>
__global__ __launch_bounds__(RS_THREADS) void gauss_kernel(Src src, long H, long W, long colblocks, const double* __restrict__ w, int radius,
                                                          double* dst) {
  const long r = (long)blockIdx.x / colblocks;   // uniform: a workgroup is RS_THREADS consecutive columns of one row
  const long c = ((long)blockIdx.x - r * colblocks) * RS_THREADS + threadIdx.x;
  if (c >= W) return;
  const long idx = r * W + c;
  double acc = src.at(idx) * w[radius];
  for (int k = 1; k <= radius; ++k) {
    const long a = AXIS == 0 ? mirror_index(r - k, H) * W + c : r * W + mirror_index(c - k, W);
    const long b = AXIS == 0 ? mirror_index(r + k, H) * W + c : r * W + mirror_index(c + k, W);
    acc += (src.at(a) + src.at(b)) * w[radius - k];
  }
  dst[idx] = acc;
}

// the anticausal value at the end `hi` of a causal run, scipy's mirror end formula: cp = c+[hi], prev = c+[hi - 1]
__device__ inline double anticausal_end(double prev, double cp) { return (POLE * prev + cp) * (POLE / (POLE * POLE - 1.0)); }

// axis 0: workgroup = RS_THREADS columns x one chunk of rows [r0, r1]; dst != src
__global__ __launch_bounds__(RS_THREADS) void prefilter_rows_kernel(Src src, long H, long W, long colblocks, double* dst) {
  const long chunk = (long)blockIdx.x / colblocks;
  const long col = ((long)blockIdx.x - chunk * colblocks) * RS_THREADS + threadIdx.x;
  if (col >= W) return;
  const long r0 = chunk * PRE_ROWS;
  const long r1 = r0 + PRE_ROWS - 1 < H - 1 ? r0 + PRE_ROWS - 1 : H - 1;
  const long hi = r1 + PRE_WARM < H - 1 ? r1 + PRE_WARM : H - 1;
  // causal warm-up: c+[r0 - 1] from the PRE_WARM rows before the chunk (rows before row 0 are mirrored)
  double c = 6.0 * src.at(mirror_index(r0 - PRE_WARM, H) * W + col);
  for (long j = r0 - PRE_WARM + 1; j < r0; ++j) c = 6.0 * src.at(mirror_index(j, H) * W + col) + POLE * c;
  double prev = c;
  for (long j = r0; j <= r1; ++j) {
    prev = c;
    c = 6.0 * src.at(j * W + col) + POLE * c;
    dst[j * W + col] = c;
  }
  double cm;   // c-[r1]
  if (r1 == H - 1) {
    cm = anticausal_end(prev, c);
  } else {
    // c-[r1 + 1] = -sum_{k < m} z^(k+1) c+[r1 + 1 + k] + z^m c-[hi], m = hi - r1 - 1, summed while the causal recursion runs on
    const double cr1 = c;
    double acc = 0.0, zp = 1.0;
    for (long j = r1 + 1; j <= hi; ++j) {
      prev = c;
      c = 6.0 * src.at(j * W + col) + POLE * c;
      if (j < hi) {
        zp *= POLE;
        acc += zp * c;
      }
    }
    const double next = zp * anticausal_end(prev, c) - acc;
    cm = POLE * (next - cr1);
  }
  dst[r1 * W + col] = cm;
  for (long j = r1 - 1; j >= r0; --j) {
    cm = POLE * (cm - dst[j * W + col]);
    dst[j * W + col] = cm;
  }
}

// axis 1: workgroup = PRE_TILE_ROWS rows x one chunk of columns [c0, c1]; the tile covers the virtual columns [c0 - PRE_WARM, hi]
__global__ __launch_bounds__(RS_THREADS) void prefilter_cols_kernel(Src src, long H, long W, long colchunks, double* dst) {
  __shared__ double tile[PRE_TILE_ROWS * PRE_STRIDE];
  const long rowblock = (long)blockIdx.x / colchunks;
  const long chunk = (long)blockIdx.x - rowblock * colchunks;
  const long row0 = rowblock * PRE_TILE_ROWS;
  const int nrows = (int)(H - row0 < PRE_TILE_ROWS ? H - row0 : PRE_TILE_ROWS);
  const long c0 = chunk * PRE_COLS;
  const long c1 = c0 + PRE_COLS - 1 < W - 1 ? c0 + PRE_COLS - 1 : W - 1;
  const long hi = c1 + PRE_WARM < W - 1 ? c1 + PRE_WARM : W - 1;
  const int span = (int)(hi - (c0 - PRE_WARM) + 1);   // <= PRE_SPAN
  for (int i = threadIdx.x; i < nrows * span; i += RS_THREADS) {
    const int tr = i / span, tc = i - tr * span;
    tile[tr * PRE_STRIDE + tc] = 6.0 * src.at((row0 + tr) * W + mirror_index(c0 - PRE_WARM + tc, W));
  }
  __syncthreads();
  if ((int)threadIdx.x < nrows) {
    double* t = tile + threadIdx.x * PRE_STRIDE;
    double c = t[0];
    for (int j = 1; j < span; ++j) {
      c = t[j] + POLE * c;
      t[j] = c;
    }
    double cm = anticausal_end(t[span - 2], c);   // (span >= PRE_WARM + 1 >= 2)
    t[span - 1] = cm;
    for (int j = span - 2; j >= PRE_WARM; --j) {
      cm = POLE * (cm - t[j]);
      t[j] = cm;
    }
  }
  __syncthreads();
  const int ncols = (int)(c1 - c0 + 1);
  for (int i = threadIdx.x; i < nrows * ncols; i += RS_THREADS) {
    const int tr = i / ncols, tc = i - tr * ncols;
    dst[(row0 + tr) * W + c0 + tc] = tile[tr * PRE_STRIDE + PRE_WARM + tc];
  }
}

template <int ORDER>
__device__ inline void zoom_axis(long o, double zoom, long n, long* idx, double* w) {
  const double c = mirror_coordinate(((double)o + 0.5) * zoom - 0.5, n);
  const double f = floor(c), t = c - f;
  const long start = (long)f - ORDER / 2;
  if (ORDER == 1) {
    w[0] = 1.0 - t;
    w[1] = t;
  } else {
    const double u = 1.0 - t;
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = u * u * u / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
  }
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) idx[k] = mirror_index(start + k, n);
}

template <int ORDER>
__global__ __launch_bounds__(RS_THREADS) void zoom_kernel(Src src, long H, long W, long out_w, long colblocks, double zy, double zx,
                                                         const double* __restrict__ lohi, float* __restrict__ out) {
  const long orow = (long)blockIdx.x / colblocks;   // uniform: a workgroup is RS_THREADS consecutive columns of one output row
  const long ocol = ((long)blockIdx.x - orow * colblocks) * RS_THREADS + threadIdx.x;
  if (ocol >= out_w) return;
  const long idx = orow * out_w + ocol;
  long ri[ORDER + 1], ci[ORDER + 1];
  double wr[ORDER + 1], wc[ORDER + 1];
  zoom_axis<ORDER>(orow, zy, H, ri, wr);
  zoom_axis<ORDER>(ocol, zx, W, ci, wc);
  double v = 0.0;
#pragma unroll
  for (int j = 0; j <= ORDER; ++j) {
    double rowsum = 0.0;
#pragma unroll
    for (int i = 0; i <= ORDER; ++i) rowsum += src.at(ri[j] * W + ci[i]) * wc[i];
    v += rowsum * wr[j];
  }
  if (lohi) v = v < lohi[0] ? lohi[0] : (v > lohi[1] ? lohi[1] : v);   // (NaN passes through, as np.clip leaves it)
  out[idx] = (float)v;
}

// roughness: tile of STD_TH x STD_TW nodes with a halo of h on every side in LDS (NaN outside the grid); thread (ty, tx) of 4 x 64
// handles the rows ty, ty + 4, ...
__global__ __launch_bounds__(RS_THREADS) void rolling_std_kernel(const float* __restrict__ in, long H, long W, int h, long colblocks,
                                                                float* __restrict__ out) {
  extern __shared__ float stile[];   // (STD_TH + 2 h) x (STD_TW + 2 h)
  const long rowblock = (long)blockIdx.x / colblocks;
  const long r0 = rowblock * STD_TH, c0 = ((long)blockIdx.x - rowblock * colblocks) * STD_TW;
  const int tw = STD_TW + 2 * h, th = STD_TH + 2 * h;
  for (int i = threadIdx.x; i < tw * th; i += RS_THREADS) {
    const int tr = i / tw, tc = i - tr * tw;
    const long r = r0 - h + tr, c = c0 - h + tc;
    stile[i] = (r >= 0 && r < H && c >= 0 && c < W) ? in[r * W + c] : __builtin_nanf("");
  }
  __syncthreads();
  const int tx = threadIdx.x & (STD_TW - 1);
  const int win = 2 * h + 1;
  for (int ty = threadIdx.x / STD_TW; ty < STD_TH; ty += RS_THREADS / STD_TW) {
    const long r = r0 + ty, c = c0 + tx;
    if (r >= H || c >= W) continue;
    const float* t = stile + ty * tw + tx;   // the window's first node
    float first = t[h * tw + h];             // the shift: the centre node, else the first valid node
    if (first != first) {
      for (int j = 0; j < win && first != first; ++j)
        for (int i = 0; i < win; ++i) {
          const float z = t[j * tw + i];
          if (z == z) { first = z; break; }
        }
    }
    float res = __builtin_nanf("");
    if (first == first) {
      const double shift = first;
      double n = 0.0, s1 = 0.0, s2 = 0.0;
      for (int j = 0; j < win; ++j)
        for (int i = 0; i < win; ++i) {
          const float z = t[j * tw + i];
          if (z == z) {
            const double d = (double)z - shift;
            n += 1.0;
            s1 += d;
            s2 += d * d;
          }
        }
      const double m = s1 / n;
      const double var = s2 / n - m * m;
      res = (float)sqrt(var > 0.0 ? var : 0.0);
    }
    out[r * W + c] = res;
  }
}

// workgroups of a launch whose workgroup is RS_THREADS consecutive columns of one row
inline unsigned row_blocks(long rows, long cols, long* colblocks) {
  *colblocks = (cols + RS_THREADS - 1) / RS_THREADS;
  DBM_CHECK(rows >= 1 && *colblocks >= 1 && *colblocks < (1L << 31) / rows, "grid rescale: too many workgroups for one launch");
  return (unsigned)(rows * *colblocks);
}

double rescale_sigma(long in, long out) {
  const double s = ((double)in / (double)out - 1.0) / 2.0;
  return s > 0.0 ? s : 0.0;
}
int gauss_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

// workspace layout in doubles: [0, 2) min / max; [2, 2 + 2 MM_BLOCKS) partials; the two axes' weights; plane A; plane B
struct RescalePlan {
  double sigma[2];
  int radius[2];
  size_t weights[2], plane[2], total;
};
RescalePlan rescale_plan(const RescaleLaunch& a) {
  RescalePlan p;
  size_t off = 2 + 2 * (size_t)MM_BLOCKS;
  const long in[2] = {a.H, a.W}, out[2] = {a.out_h, a.out_w};
  bool filtered = false;
  for (int k = 0; k < 2; ++k) {
    p.sigma[k] = a.anti_aliasing ? rescale_sigma(in[k], out[k]) : 0.0;
    p.radius[k] = gauss_radius(p.sigma[k]);
    p.weights[k] = off;
    if (p.sigma[k] > 0.0) {
      off += 2 * (size_t)p.radius[k] + 1;
      filtered = true;
    }
  }
  const size_t hw = (size_t)a.H * (size_t)a.W;
  const int planes = (a.order == 3 || filtered) ? 2 : 0;
  for (int k = 0; k < 2; ++k) {
    p.plane[k] = off;
    off += planes ? hw : 0;
  }
  p.total = off;
  return p;
}

}  // namespace

size_t grid_rescale_workspace(const RescaleLaunch& a) { return rescale_plan(a).total; }

void launch_grid_rescale(const RescaleLaunch& a, hipStream_t s) {
  const RescalePlan p = rescale_plan(a);
  const long hw = a.H * a.W;
  Src cur{a.in, nullptr, a.input_cast};
  if (a.clip) {
    const long b = (hw + RS_THREADS - 1) / RS_THREADS;
    const int blocks = (int)(b < MM_BLOCKS ? b : MM_BLOCKS);
    hipLaunchKernelGGL(minmax_kernel, dim3(blocks), dim3(RS_THREADS), 0, s, cur, hw, a.ws + 2);
    DBM_HIP(hipGetLastError());
    hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(RS_THREADS), 0, s, a.ws + 2, blocks, a.ws);
    DBM_HIP(hipGetLastError());
  }
  int next = 0;   // the plane the next pass writes
  auto advance = [&]() {
    cur = Src{nullptr, a.ws + p.plane[next], 0};
    next ^= 1;
  };
  long plane_colblocks = 0;
  const unsigned plane_blocks = row_blocks(a.H, a.W, &plane_colblocks);
  for (int k = 0; k < 2; ++k) {
    if (!(p.sigma[k] > 0.0)) continue;
    double* w = a.ws + p.weights[k];
    hipLaunchKernelGGL(gauss_weights_kernel, dim3(1), dim3(RS_THREADS), 0, s, p.sigma[k], p.radius[k], w);
    DBM_HIP(hipGetLastError());
    if (k == 0)
      hipLaunchKernelGGL(gauss_kernel<0>, dim3(plane_blocks), dim3(RS_THREADS), 0, s, cur, a.H, a.W, plane_colblocks, w, p.radius[k],
                         a.ws + p.plane[next]);
    else
      hipLaunchKernelGGL(gauss_kernel<1>, dim3(plane_blocks), dim3(RS_THREADS), 0, s, cur, a.H, a.W, plane_colblocks, w, p.radius[k],
                         a.ws + p.plane[next]);
    DBM_HIP(hipGetLastError());
    advance();
  }
  if (a.order == 3) {
    const long colblocks = (a.W + RS_THREADS - 1) / RS_THREADS, rowchunks = (a.H + PRE_ROWS - 1) / PRE_ROWS;
    DBM_CHECK(colblocks * rowchunks < (1L << 31), "grid rescale: too many workgroups for one launch");
    hipLaunchKernelGGL(prefilter_rows_kernel, dim3((unsigned)(colblocks * rowchunks)), dim3(RS_THREADS), 0, s, cur, a.H, a.W, colblocks,
                       a.ws + p.plane[next]);
    DBM_HIP(hipGetLastError());
    advance();
    const long colchunks = (a.W + PRE_COLS - 1) / PRE_COLS, rowblocks = (a.H + PRE_TILE_ROWS - 1) / PRE_TILE_ROWS;
    DBM_CHECK(colchunks * rowblocks < (1L << 31), "grid rescale: too many workgroups for one launch");
    hipLaunchKernelGGL(prefilter_cols_kernel, dim3((unsigned)(colchunks * rowblocks)), dim3(RS_THREADS), 0, s, cur, a.H, a.W, colchunks,
                       a.ws + p.plane[next]);
    DBM_HIP(hipGetLastError());
    advance();
  }
  long out_colblocks = 0;
  const unsigned out_blocks = row_blocks(a.out_h, a.out_w, &out_colblocks);
  const double zy = (double)a.H / (double)a.out_h, zx = (double)a.W / (double)a.out_w;
  const double* lohi = a.clip ? a.ws : nullptr;
  if (a.order == 1)
    hipLaunchKernelGGL(zoom_kernel<1>, dim3(out_blocks), dim3(RS_THREADS), 0, s, cur, a.H, a.W, a.out_w, out_colblocks, zy, zx, lohi,
                       a.out);
  else
    hipLaunchKernelGGL(zoom_kernel<3>, dim3(out_blocks), dim3(RS_THREADS), 0, s, cur, a.H, a.W, a.out_w, out_colblocks, zy, zx, lohi,
                       a.out);
  DBM_HIP(hipGetLastError());
}

void launch_rolling_std(const float* in, long H, long W, int window, float* out, hipStream_t s) {
  const int h = window / 2;
  const long colblocks = (W + STD_TW - 1) / STD_TW, rowblocks = (H + STD_TH - 1) / STD_TH;
  DBM_CHECK(colblocks * rowblocks < (1L << 31), "rolling standard deviation: too many workgroups for one launch");
  const size_t lds = sizeof(float) * (size_t)(STD_TW + 2 * h) * (size_t)(STD_TH + 2 * h);   // <= 39 312 bytes (window 63)
  hipLaunchKernelGGL(rolling_std_kernel, dim3((unsigned)(colblocks * rowblocks)), dim3(RS_THREADS), lds, s, in, H, W, h, colblocks, out);
  DBM_HIP(hipGetLastError());
}
