// The overview pyramid of a resident plane (dbm_grid_overviews; the host side -- directories, container, batching -- is
// deepbedmap_amd/geotiff.py).  Reference: deepbedmap.py:749-756 saves the stitched DEM through data_prep.py:779-834 (rasterio / GDAL) as
// one full-resolution image; every reader of that file then runs `gdaladdo -r average` on it.  This file builds those reduced images
// next to the canvas, so that still only compressed bytes cross PCIe.  DESIGN.md 6j, "Overviews".
//
// The definition (this project's own, exact; `gdaladdo -r average` in spirit).  Level 0 is the image as written: the plane's samples
// after the cast to the file's type (int16: dbm_cast_i16, kernels.h; float32: the bits).  Level k + 1 is made from level k alone:
//   shape     H' = ceil(H / 2), W' = ceil(W / 2);
//   window    pixel (r, c) covers source rows 2r, 2r + 1 and columns 2c, 2c + 1 as far as they exist (2 samples or 1 at an odd edge);
//   validity  float32 files: a source sample is valid unless it is NaN or equals float32(nodata); int16 files: unless it equals
//             int(nodata);
//   sum       s = (a00 + a01) + (a10 + a11) in float32, samples that are invalid or do not exist entering as +0.0f;
//   count     n = the number of valid samples;
//   mean      m = s / float32(n): one IEEE single-precision division (no reciprocal; this file is never compiled with fast-math);
//   result    n == 0: nodata (float32(nodata) / int(nodata)); else float32 files: m; int16 files: rint(m), ties to even, and the next
//             level is made from these rounded samples.
// int16 samples travel as exactly representable floats (0 always as +0.0f), so dbm_tiff_encode encodes a level unchanged (its cast is then the identity).
//
// Decomposition.  One workgroup of 256 threads owns a 64 x 64 source tile whose origin is a multiple of 64 -- hence of 8, so the three
// halvings inside a tile are the global ones -- and writes its 32 x 32, 16 x 16 and 8 x 8 results in one launch: one pass over memory
// per THREE levels.  Deeper levels repeat the launch on the third result (a 64th of the samples).
//   level 1   thread t takes the float4 column q = t % 16 of the row pairs p = t / 16 and t / 16 + 16: four 16-byte loads (16 lanes read
//             256 contiguous bytes of a row; scalar loads where W % 4 != 0 or at a ragged edge), two results per pair from registers.
//   level 2   from LDS.  Level 1 lies there as 32 rows of 48 floats: thread (r, c) = (t / 16, t % 16) reads the float2 at
//             (2r, 2c) and at (2r + 1, 2c).  A 32-lane group of that 8-byte read spans two values of r; its bank is (a / 4) % 64, and
//             with a row stride of 48 the second r starts 96 = 32 (mod 64) dwords on: the two halves tile the 64 banks.  (Stride 32
//             would put both on banks 0..31: 2-way.)  The level-1 float2 writes are 16 lanes on 32 consecutive dwords: conflict free.
//   level 3   from LDS, one wavefront.  Level 2 lies there as 16 rows of 24 floats: lane (r, c) = (l / 8, l % 8) reads float2s at
//             (2r, 2c), (2r + 1, 2c); a 32-lane group spans four values of r, 48 dwords apart: offsets 0, 48, 32, 16 (mod 64), 16
//             dwords each: conflict free.
// A sample that does not exist (right of or below its level) is carried as NaN: invalid in either file type, it adds +0.0f and
// does not count, which is what the definition asks of it.
#include "kernels.h"

namespace {

constexpr int PYR_THREADS = 256;
constexpr int PYR_TILE = 64;
constexpr int PYR_S1 = 48;   // floats per row of the 32 x 32 level in LDS
constexpr int PYR_S2 = 24;   // floats per row of the 16 x 16 level in LDS

struct PyramidArgs {
  const float* src;
  long H, W;                 // the source level
  float* out[3];             // the next levels, (H + 1) / 2 x (W + 1) / 2 and so on
  int nlev;                  // 1..3 of them
  int cast;                  // the source is the canvas of an int16 file: dbm_cast_i16 while reading
  int round;                 // int16 file: rint
  float nodata;              // float32(nodata) / float(int(nodata)): the invalid value, and the result of an empty window
  long tiles_x;
};

__device__ __forceinline__ float pyr_mean(float a00, float a01, float a10, float a11, float nd, int round) {
  const bool v00 = a00 == a00 && a00 != nd, v01 = a01 == a01 && a01 != nd;
  const bool v10 = a10 == a10 && a10 != nd, v11 = a11 == a11 && a11 != nd;
  const float s = ((v00 ? a00 : 0.f) + (v01 ? a01 : 0.f)) + ((v10 ? a10 : 0.f) + (v11 ? a11 : 0.f));
  const int n = (int)v00 + (int)v01 + (int)v10 + (int)v11;
  if (n == 0) return nd;
  const float m = s / (float)n;
  return round ? rintf(m) + 0.f : m;   // (+ 0.f: a mean in [-0.5, -0] is the int16 sample 0, stored as +0.0f, not -0.0f)
}

// four samples of row `row` from column `col` (a multiple of 4); NaN where the plane has none
__device__ __forceinline__ float4 pyr_load4(const PyramidArgs& a, long row, long col, bool vec) {
  const float none = __builtin_nanf("");
  float4 v = make_float4(none, none, none, none);
  if (row >= a.H || col >= a.W) return v;
  const float* p = a.src + row * a.W + col;
  if (vec) {   // (W % 4 == 0: the four columns exist)
    v = *reinterpret_cast<const float4*>(p);
  } else {
    v.x = p[0];
    if (col + 1 < a.W) v.y = p[1];
    if (col + 2 < a.W) v.z = p[2];
    if (col + 3 < a.W) v.w = p[3];
  }
  if (a.cast) {
    v.x = (float)dbm_cast_i16(v.x);
    if (vec || col + 1 < a.W) v.y = (float)dbm_cast_i16(v.y);
    if (vec || col + 2 < a.W) v.z = (float)dbm_cast_i16(v.z);
    if (vec || col + 3 < a.W) v.w = (float)dbm_cast_i16(v.w);
  }
  return v;
}

__global__ __launch_bounds__(PYR_THREADS) void pyramid_kernel(PyramidArgs a) {
  __shared__ __attribute__((aligned(16))) float s1[32 * PYR_S1];
  __shared__ __attribute__((aligned(16))) float s2[16 * PYR_S2];
  const float none = __builtin_nanf("");
  const int t = threadIdx.x;
  const long ty = (long)blockIdx.x / a.tiles_x, tx = (long)blockIdx.x % a.tiles_x;
  const long H1 = (a.H + 1) / 2, W1 = (a.W + 1) / 2;
  const bool vec = a.W % 4 == 0 && ((size_t)a.src & 15) == 0;   // (the same for every thread)

  // ---- level 1: registers ----
  {
    const int q = t & 15, p0 = t >> 4;
    const long col = tx * PYR_TILE + 4 * q;
    float4 x[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long row = ty * PYR_TILE + 2 * (p0 + 16 * j);
      x[j][0] = pyr_load4(a, row, col, vec);
      x[j][1] = pyr_load4(a, row + 1, col, vec);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = p0 + 16 * j;
      const long r1 = ty * (PYR_TILE / 2) + p, c1 = tx * (PYR_TILE / 2) + 2 * q;
      float2 o;
      o.x = r1 < H1 && c1 < W1 ? pyr_mean(x[j][0].x, x[j][0].y, x[j][1].x, x[j][1].y, a.nodata, a.round) : none;
      o.y = r1 < H1 && c1 + 1 < W1 ? pyr_mean(x[j][0].z, x[j][0].w, x[j][1].z, x[j][1].w, a.nodata, a.round) : none;
      *reinterpret_cast<float2*>(&s1[p * PYR_S1 + 2 * q]) = o;
      if (r1 < H1 && c1 < W1) {
        float* dst = a.out[0] + r1 * W1 + c1;
        if (c1 + 1 < W1 && ((size_t)dst & 7) == 0) {
          *reinterpret_cast<float2*>(dst) = o;
        } else {
          dst[0] = o.x;
          if (c1 + 1 < W1) dst[1] = o.y;
        }
      }
    }
  }
  if (a.nlev < 2) return;   // (nlev is the launch's: no thread waits at a barrier another one skips)
  __syncthreads();

  // ---- level 2: one result per thread, from the 32 x 32 level in LDS ----
  const long H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2;
  {
    const int r = t >> 4, c = t & 15;
    const float2 u = *reinterpret_cast<const float2*>(&s1[(2 * r) * PYR_S1 + 2 * c]);
    const float2 d = *reinterpret_cast<const float2*>(&s1[(2 * r + 1) * PYR_S1 + 2 * c]);
    const long r2 = ty * (PYR_TILE / 4) + r, c2 = tx * (PYR_TILE / 4) + c;
    const bool exists = r2 < H2 && c2 < W2;
    const float o = exists ? pyr_mean(u.x, u.y, d.x, d.y, a.nodata, a.round) : none;
    s2[r * PYR_S2 + c] = o;
    if (exists) a.out[1][r2 * W2 + c2] = o;
  }
  if (a.nlev < 3) return;
  __syncthreads();

  // ---- level 3: the first wavefront, from the 16 x 16 level in LDS ----
  if (t < 64) {
    const long H3 = (H2 + 1) / 2, W3 = (W2 + 1) / 2;
    const int r = t >> 3, c = t & 7;
    const float2 u = *reinterpret_cast<const float2*>(&s2[(2 * r) * PYR_S2 + 2 * c]);
    const float2 d = *reinterpret_cast<const float2*>(&s2[(2 * r + 1) * PYR_S2 + 2 * c]);
    const long r3 = ty * (PYR_TILE / 8) + r, c3 = tx * (PYR_TILE / 8) + c;
    if (r3 < H3 && c3 < W3) a.out[2][r3 * W3 + c3] = pyr_mean(u.x, u.y, d.x, d.y, a.nodata, a.round);
  }
}

}  // namespace

int pyramid_max_levels(long H, long W) {
  int n = 0;
  while (H > 1 || W > 1) {
    H = (H + 1) / 2;
    W = (W + 1) / 2;
    ++n;
  }
  return n;
}

void launch_grid_overviews(const PyramidLaunch& l, hipStream_t s) {
  PyramidArgs a;
  a.src = l.plane;
  a.H = l.H;
  a.W = l.W;
  a.cast = l.sample_type == 1;
  a.round = l.sample_type == 1;
  a.nodata = l.nodata;
  float* dst = l.out;
  for (int done = 0; done < l.levels; done += 3) {
    a.nlev = l.levels - done < 3 ? l.levels - done : 3;
    long h = a.H, w = a.W;
    for (int k = 0; k < 3; ++k) {   // (levels beyond nlev are never written: their pointers only keep the struct defined)
      h = (h + 1) / 2;
      w = (w + 1) / 2;
      a.out[k] = dst;
      if (k < a.nlev) dst += h * w;
    }
    a.tiles_x = (a.W + PYR_TILE - 1) / PYR_TILE;
    const long tiles = a.tiles_x * ((a.H + PYR_TILE - 1) / PYR_TILE);   // H W < 2^31: at most 2^25
    hipLaunchKernelGGL(pyramid_kernel, dim3((unsigned)tiles), dim3(PYR_THREADS), 0, s, a);
    DBM_HIP(hipGetLastError());
    a.src = a.out[2];   // the next launch halves the third result
    a.H = h;
    a.W = w;
    a.cast = 0;
  }
}
