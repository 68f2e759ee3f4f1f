// What the fused deformable kernels share (deform_fwd.hip, deform_window.hip, deform_bwd.hip): the 64-position tile and its corner
// table, the sampler's corner request and blend, the sample-tile write and the 64 -> 64 epilogue -- one copy of each.  These kernels are
// scheduled by hand: a piece is shared only where the kernel compiles to the instructions it had with its own copy
// (tools/kernel_isa.py before and after), in the shape that does -- a function where that holds, a macro where only the
// same tokens do -- and a kernel that matches in neither shape keeps its copy, marked with a comment naming the piece.
#pragma once
#include <hip/hip_runtime.h>
#include "deform_geom.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 dbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dbf16x4 __attribute__((ext_vector_type(4)));

constexpr int DF_POS = 64;   // positions per workgroup
constexpr int DF_LD = 65;    // LDS row stride of the sample tile [channel][position] (odd: conflict-free column access)

// Corner table of a 64-position tile: for (tap t, position pl) the four pixel indices n * plane + offset into the
// channels-last copy and the four bilinear weights; a corner outside the image keeps index 0 with weight 0.
struct TileGeometry {
  int4 idx[9 * DF_POS];
  float4 wgt[9 * DF_POS];
};

// taps [t_lo, t_hi) of the table, dealt to 256 threads.
// (t_lo / t_hi by reference: in a file whose every caller passes the same constants, by value they are propagated into this body BEFORE
//  it is inlined, and the forward kernels then compile to other instructions than beside deform_wgrad64_fused_kernel's run-time bounds)
__device__ __forceinline__ void build_geometry(TileGeometry& g, const float* __restrict__ off, long offsn, long P0, long total, int plane,
                                               int H, int W, int tid, int abl = 0, const int& t_lo = 0, const int& t_hi = 9) {
  for (int e = t_lo * DF_POS + tid; e < t_hi * DF_POS; e += 256) {
    const int t = e >> 6, pl = e & 63;
    const long P = P0 + pl;
    int4 id = make_int4(0, 0, 0, 0);
    float4 wg = make_float4(0.f, 0.f, 0.f, 0.f);
    if (P < total) {
      const int n = (int)(P / plane);
      const int p = (int)(P - (long)n * plane);
      const int a = p / W, b = p - a * W;
      const float* on = off + (long)n * offsn;
      const DeformTap s = deform_tap(on[(long)t * plane + p], on[(long)(9 + t) * plane + p], a, b, t / 3, t % 3, H, W);
      const int base = n * plane;
      if (s.o1 >= 0) { id.x = base + s.o1; wg.x = s.w1(); }
      if (s.o2 >= 0) { id.y = base + s.o2; wg.y = s.w2(); }
      if (s.o3 >= 0) { id.z = base + s.o3; wg.z = s.w3(); }
      if (s.o4 >= 0) { id.w = base + s.o4; wg.w = s.w4(); }
      if (abl) id = make_int4(base, base, base, base);   // (libdbm_measure.so only: every gather hits one cache-resident pixel)
    }
    g.idx[e] = id;
    g.wgt[e] = wg;
  }
}

__device__ __forceinline__ float4 blend4(const float4& w, const float4& a, const float4& b, const float4& c, const float4& d) {
  float4 r;
  r.x = w.x * a.x + w.y * b.x + w.z * c.x + w.w * d.x;
  r.y = w.x * a.y + w.y * b.y + w.z * c.y + w.w * d.y;
  r.z = w.x * a.z + w.y * b.z + w.z * c.z + w.w * d.z;
  r.w = w.x * a.w + w.y * b.w + w.z * c.w + w.w * d.w;
  return r;
}

// The sampler role of a 256-thread workgroup: lane = (position lane >> 4 = pi, channel quad lane & 15 = q), wavefront `wave` owns
// positions 16 wave .. 16 wave + 15 in four steps i: position 16 wave + 4 i + pi.  A request is in flight until its values are used.
struct CornerRequest {
  float4 c1[4], c2[4], c3[4], c4[4], cw[4];
  // requests the four corners of this lane's channel quad at its four positions (xq = xt + 4 q)
  __device__ __forceinline__ void request(const TileGeometry& geo, const float* xq, int t, int wave, int pi) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t * DF_POS + 16 * wave + 4 * i + pi;
      const int4 id = geo.idx[e];
      cw[i] = geo.wgt[e];
      c1[i] = *reinterpret_cast<const float4*>(xq + (long)id.x * 64);
      c2[i] = *reinterpret_cast<const float4*>(xq + (long)id.y * 64);
      c3[i] = *reinterpret_cast<const float4*>(xq + (long)id.z * 64);
      c4[i] = *reinterpret_cast<const float4*>(xq + (long)id.w * 64);
    }
  }
  __device__ __forceinline__ float4 blended(int i) const { return blend4(cw[i], c1[i], c2[i], c3[i], c4[i]); }
  // the blended samples into a [channel][position] fp32 LDS tile (row stride DF_LD)
  __device__ __forceinline__ void write_samples(float* dst, int q, int wave, int pi) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = blended(i);
      float* d = dst + (4 * q) * DF_LD + 16 * wave + 4 * i + pi;
      d[0] = v.x; d[DF_LD] = v.y; d[2 * DF_LD] = v.z; d[3 * DF_LD] = v.w;
    }
  }
};

// ---- epilogue of the 64 -> 64 forwards: bias, LeakyReLU; y in 128-byte runs along the position axis, yt (channels-last) as 16-byte
// channel quads.  A lane (position, k half kh) of the wavefront that owns output-channel tile ct holds, in accumulator register r,
// channel ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh. ----
#define DF_ACC_ROW(ct, kh, r) ((ct) * 32 + ((r) & 3) + 8 * ((r) >> 2) + 4 * (kh))

// v[r] = act(acc[r] + bias[channel of r]), r = 0..15.  A macro: as a function -- taking the tile by reference or by value, or one value
// at a time -- this loop compiled to other branches around the bias loads in every kernel that uses it.
// (round 5: every bias value is loaded BEFORE the first store -- vmcnt counts stores too, in order, so a load behind a store is
//  awaited by draining the store: the interleaved form paid sixteen write round trips per thread)
#define DF_EPILOGUE64_VALUES(v, acc, ct, kh, bias, act, slope)     \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) {                 \
    const int c = DF_ACC_ROW(ct, kh, r);                           \
    (v)[r] = (acc)[r] + ((bias) ? (bias)[c] : 0.f);                \
    if (act) (v)[r] = (v)[r] >= 0.f ? (v)[r] : (slope) * (v)[r];   \
  }
// the y stores of those values: y[yoff] = channel 0 of the lane's position, yoff = (n * 64) * plane + p
#define DF_EPILOGUE64_STORE_Y(v, ct, kh, y, yoff, plane) \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) (y)[(yoff) + (long)DF_ACC_ROW(ct, kh, r) * (plane)] = (v)[r];
// the yt stores: ytp = yt + (n * plane + p) * 64, the lane's pixel
#define DF_EPILOGUE64_STORE_YT(v, ct, kh, ytp)       \
  _Pragma("unroll") for (int g = 0; g < 4; ++g)      \
    *reinterpret_cast<float4*>((ytp) + (ct) * 32 + 8 * g + 4 * (kh)) = make_float4((v)[4 * g], (v)[4 * g + 1], (v)[4 * g + 2], (v)[4 * g + 3]);
