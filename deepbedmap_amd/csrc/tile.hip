// Cutting tiles from resident rasters (reference data_prep.py:501-572 `get_window_bounds`, :622-741 `selective_tile`; deepbedmap.py:132-213
// `get_deepbedmap_model_inputs` cuts the four inputs of an area with the same function).  Two kernels, 64-bit element offsets everywhere,
// launch geometry a function of the problem size only (DESIGN.md "Tiling"):
//
// grid_tile_kernel -- one lane per output value, lanes running along out_w.  Window k = (left, bottom, right, top), already padded:
//   - output coordinates: np.linspace(top - res/2, bottom + res/2, out_h) and np.linspace(left + res/2, right - res/2, out_w) in float64,
//     bit-equal to NumPy: start + i * step as a rounded multiply and a rounded add (never fused), the last element = stop;
//   - bilinear (mode 1), scipy's rule (`xarray.DataArray.interp(method="linear")` -> scipy.interpolate.interpn): each axis ascending, node
//     coordinates g[i] = x0 + j dx (multiply, then add), the cell i with g[i] <= c < g[i+1] (the last node: i = n - 2, t = 1),
//     t = (c - g[i]) / (g[i+1] - g[i]); c < g[0], c > g[n-1] or NaN: NaN; the value is the float64 sum of z * (wy * wx) over ALL four
//     nodes in the order (i, j), (i, j+1), (i+1, j), (i+1, j+1), zero weights included (0 * NaN = NaN);
//   - slicing (mode 0, `sel(method="nearest", tolerance=0)` after the host has checked that every coordinate IS a node): window k =
//     (row0, col0, row step, column step) as int64, a pure copy;
//   - masking (numpy.ma.masked_values after the interpolation): v masked iff |v - nodata| <= 1e-8 + 1e-5 |nodata|; NaN results are not
//     masked unless fill_nan; masked values become the gap filler if there is one; optional int32 count of masked values per window;
//   - rounded to float32 once, at the end.
//
// filled_rows_kernel + filled_windows_kernel -- the separable form of "no NaN in the size x size window (uly step, ulx step)": the row pass
// stages a row segment's NaN flags in LDS and writes, per row and window column, whether the row's `size` nodes hold a NaN (each raster
// element is read from HBM once, plus the segments' overlap); the column pass ORs `size` of those bytes per window (the byte plane is
// 1 / (4 step) of the raster's bytes and is read size / step times).
#include "model.h"
#include <cmath>

// NumPy and scipy round every product and every sum: nothing in this file may be contracted into a fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int TILE_THREADS = 256;
constexpr int ROWSEG_THREADS = 256;

// v[i] of np.linspace(start, stop, num): arange(num) * step + start, the end point stored exactly
__device__ inline double linspace_at(double start, double stop, int num, int i) {
  if (num == 1) return start;
  if (i == num - 1) return stop;
  const double step = (stop - start) / (double)(num - 1);
  return (double)i * step + start;
}

// coordinate of raster index j: x0 + j dx, multiply then add
__device__ inline double node_at(double x0, double dx, long j) { return (double)j * dx + x0; }

// The cell of c on the axis sorted ascending: a = index of g[i] in raster order, b = index of g[i+1], t = the normalised distance.
// false: c lies outside [g[0], g[n-1]] or is NaN.
__device__ inline bool find_cell(double c, double x0, double dx, long n, long* a, long* b, double* t) {
  const bool up = dx > 0.0;
  const double lo = up ? x0 : node_at(x0, dx, n - 1), hi = up ? node_at(x0, dx, n - 1) : x0;
  if (!(c >= lo && c <= hi)) return false;
  // ascending index i <-> raster index j = up ? i : n - 1 - i
  const double est = floor((c - lo) / fabs(dx));
  long i = est < 0.0 ? 0 : (est > (double)(n - 2) ? n - 2 : (long)est);
  double gi = node_at(x0, dx, up ? i : n - 1 - i);
  while (i > 0 && c < gi) {          // the estimate is at most a rounding away: these loops run once at the most
    --i;
    gi = node_at(x0, dx, up ? i : n - 1 - i);
  }
  double gn = node_at(x0, dx, up ? i + 1 : n - 2 - i);
  while (i < n - 2 && c >= gn) {
    ++i;
    gi = gn;
    gn = node_at(x0, dx, up ? i + 1 : n - 2 - i);
  }
  *a = up ? i : n - 1 - i;
  *b = up ? i + 1 : n - 2 - i;
  *t = (c - gi) / (gn - gi);
  return true;
}

// Mode 1: the raster at row r, column c of the window w = (left, bottom, right, top), in float64 (NaN outside the raster)
__device__ inline double tile_bilinear(const TileLaunch& a, const double* w, int r, int c) {
  const double half = a.res * 0.5;
  const double y = linspace_at(w[3] - half, w[1] + half, a.out_h, r);
  const double x = linspace_at(w[0] + half, w[2] - half, a.out_w, c);
  long r0, r1, c0, c1;
  double ty, tx;
  double v = __builtin_nan("");
  if (find_cell(y, a.y0, a.dy, a.H, &r0, &r1, &ty) && find_cell(x, a.x0, a.dx, a.W, &c0, &c1, &tx)) {
    const float* p0 = a.grid + r0 * a.W;
    const float* p1 = a.grid + r1 * a.W;
    const double z00 = p0[c0], z01 = p0[c1], z10 = p1[c0], z11 = p1[c1];
    const double uy = 1.0 - ty, ux = 1.0 - tx;
    v = 0.0 + z00 * (uy * ux);   // (scipy starts from 0.: a first term of -0.0 becomes +0.0)
    v = v + z01 * (uy * tx);
    v = v + z10 * (ty * ux);
    v = v + z11 * (ty * tx);
  }
  return v;
}

template <int MODE>
__global__ __launch_bounds__(TILE_THREADS) void grid_tile_kernel(TileLaunch a) {
  const long idx = (long)blockIdx.x * TILE_THREADS + threadIdx.x;
  const long hw = (long)a.out_h * a.out_w;
  const bool live = idx < a.n * hw;
  long k = 0;
  bool masked = false;
  if (live) {
    k = idx / hw;
    const int p = (int)(idx - k * hw);
    const int r = p / a.out_w, c = p - r * a.out_w;
    double v;
    if (MODE == 0) {
      const long* w = (const long*)a.windows + 4 * k;
      const long rr = w[0] + (long)r * w[2], cc = w[1] + (long)c * w[3];   // (inside the raster: checked on the host for every window)
      v = (double)a.grid[rr * a.W + cc];
    } else {
      v = tile_bilinear(a, (const double*)a.windows + 4 * k, r, c);
    }
    if (a.has_nodata) masked = fabs(v - a.nodata) <= a.nodata_band;   // (false for NaN v)
    if (a.fill_nan && v != v) masked = true;
    float o = (float)v;
    if (masked && a.has_fill) o = a.fill;
    a.out[k * a.out_stride + p] = o;
  }
  if (a.counts) {
    // one integer atomic per wave where the wave lies inside one window, one per masked lane otherwise: exact either way
    const long k0 = (long)__shfl((long long)k, 0, 64);
    const bool uniform = __all(!live || k == k0);
    const unsigned long long m = __ballot(masked);
    if (uniform) {
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.counts + k0, (int)__popcll(m));
    } else if (masked) {
      atomicAdd(a.counts + k, 1);
    }
  }
}

// dbm_grid_fill_gaps: one lane per node of the fine raster = of the one tile that grid_tile_kernel<1> would cut from the coarse raster
struct FillWindow { double w[4]; };
__global__ __launch_bounds__(TILE_THREADS) void grid_fill_gaps_kernel(TileLaunch a, FillWindow win, const float* fine, int has_fine_nodata,
                                                                      float fine_nodata, float* out) {
  const long idx = (long)blockIdx.x * TILE_THREADS + threadIdx.x;
  if (idx >= (long)a.out_h * a.out_w) return;
  const float z = fine[idx];
  const bool gap = z != z || (has_fine_nodata && z == fine_nodata);
  float o = z;
  if (gap) {
    const long r = idx / a.out_w;
    o = (float)tile_bilinear(a, win.w, (int)r, (int)(idx - r * a.out_w));
  }
  if (gap || out != fine) ((unsigned*)out)[idx] = __float_as_uint(o);   // (nodes with data: the same bits)
}

// Row pass: block (segment sgm of logical row lr) -> rowany[lr * nx + ulx] = 1 iff a node of columns [ulx step, ulx step + size) of
// that row is NaN, for the segment's window columns ulx in [sgm * nw, min(nx, (sgm + 1) * nw)).  Logical rows count from the north,
// logical columns from the west.
__global__ __launch_bounds__(ROWSEG_THREADS) void filled_rows_kernel(FilledLaunch a) {
  extern __shared__ unsigned char nanflag[];   // (nw - 1) * step + size bytes
  const long lr = (long)blockIdx.x / a.nseg;
  const long sgm = (long)blockIdx.x - lr * a.nseg;
  const long ulx0 = sgm * a.nw;
  const long nwin = a.nx - ulx0 < a.nw ? a.nx - ulx0 : a.nw;
  const long col0 = ulx0 * a.step;
  const int ncol = (int)((nwin - 1) * a.step + a.size);   // col0 + ncol <= (nx - 1) step + size <= W
  const float* row = a.grid + (a.flip_rows ? a.H - 1 - lr : lr) * a.W;
  for (int i = threadIdx.x; i < ncol; i += ROWSEG_THREADS) {
    const long lc = col0 + i;
    const float z = row[a.flip_cols ? a.W - 1 - lc : lc];
    nanflag[i] = z != z;
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nwin; w += ROWSEG_THREADS) {
    const unsigned char* f = nanflag + (long)w * a.step;
    unsigned char any = 0;
    for (int j = 0; j < a.size; ++j) any |= f[j];
    a.rowany[lr * a.nx + ulx0 + w] = any;
  }
}

// Column pass: one lane per window (uly, ulx), lanes along ulx: flag = no NaN in rows [uly step, uly step + size)
__global__ __launch_bounds__(TILE_THREADS) void filled_windows_kernel(FilledLaunch a) {
  const long idx = (long)blockIdx.x * TILE_THREADS + threadIdx.x;
  if (idx >= a.ny * a.nx) return;
  const long uly = idx / a.nx, ulx = idx - uly * a.nx;
  const unsigned char* p = a.rowany + uly * a.step * a.nx + ulx;   // last row read: (ny - 1) step + size - 1 < rows
  unsigned char any = 0;
  for (int j = 0; j < a.size; ++j) any |= p[(long)j * a.nx];
  a.flags[idx] = any ? 0 : 1;
}

}  // namespace

void launch_grid_tile(const TileLaunch& a, hipStream_t s) {
  const long total = a.n * (long)a.out_h * a.out_w;
  if (total <= 0) return;
  const long blocks = (total + TILE_THREADS - 1) / TILE_THREADS;
  DBM_CHECK(blocks < (1L << 31), "grid tiling: more than 2^39 output values in one call");
  if (a.mode == 0)
    hipLaunchKernelGGL(grid_tile_kernel<0>, dim3((unsigned)blocks), dim3(TILE_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(grid_tile_kernel<1>, dim3((unsigned)blocks), dim3(TILE_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_grid_fill_gaps(const TileLaunch& a, const double window[4], const float* fine, int has_fine_nodata, float fine_nodata, float* out,
                           hipStream_t s) {
  const long total = (long)a.out_h * a.out_w;
  if (total <= 0) return;
  const long blocks = (total + TILE_THREADS - 1) / TILE_THREADS;
  DBM_CHECK(blocks < (1L << 31), "gap filling: more than 2^39 nodes in one call");
  FillWindow win;
  for (int k = 0; k < 4; ++k) win.w[k] = window[k];
  hipLaunchKernelGGL(grid_fill_gaps_kernel, dim3((unsigned)blocks), dim3(TILE_THREADS), 0, s, a, win, fine, has_fine_nodata, fine_nodata, out);
  DBM_HIP(hipGetLastError());
}

void filled_windows_geometry(FilledLaunch& a) {
  a.ny = (a.H - a.size) / a.step + 1;
  a.nx = (a.W - a.size) / a.step + 1;
  a.rows = (a.ny - 1) * a.step + a.size;
  const long fit = (FILLED_LDS_BYTES - a.size) / a.step + 1;   // windows whose columns fit the LDS segment
  a.nw = fit < ROWSEG_THREADS ? fit : ROWSEG_THREADS;
  a.nseg = (a.nx + a.nw - 1) / a.nw;
}

void launch_filled_windows(const FilledLaunch& a, hipStream_t s) {
  const long row_blocks = a.rows * a.nseg;
  const long win_blocks = (a.ny * a.nx + TILE_THREADS - 1) / TILE_THREADS;
  DBM_CHECK(row_blocks < (1L << 31) && win_blocks < (1L << 31), "filled-window search: too many workgroups for one launch");
  const size_t lds = (size_t)((a.nw - 1) * a.step + a.size);
  hipLaunchKernelGGL(filled_rows_kernel, dim3((unsigned)row_blocks), dim3(ROWSEG_THREADS), lds, s, a);
  DBM_HIP(hipGetLastError());
  hipLaunchKernelGGL(filled_windows_kernel, dim3((unsigned)win_blocks), dim3(TILE_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}
