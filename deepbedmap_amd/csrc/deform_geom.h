// Sampling geometry of the deformable convolution (reference srgan_train.py:506-523, :572-574; Chainer
// deformable_convolution_2d_sampler + spatial_transformer_sampler semantics), shared by the sampler
// kernels of deform_sampler.hip and the fused sampler + GEMM kernels of deform_fwd.hip, deform_window.hip and deform_bwd.hip.  Every kernel takes a sample's corners,
// weights and coordinate gradients from here: the sequence of single float32 operations below IS the reference's (a coordinate next
// to an integer lands on the side its rounding decides; tests/test_deform_cases_host.py shows what another sequence costs).
#pragma once
#include <hip/hip_runtime.h>

struct DeformGeom {
  int u0, v0;            // top-left corner in the sampler's doubly padded frame
  float wu0, wu1, wv0, wv1;
  bool mu, mv;           // coordinate-gradient masks (not clipped)
};

__device__ __forceinline__ DeformGeom deform_geom(float offx, float offy, int a, int b, int ky, int kx, int H, int W,
                                                  int pad) {
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  // _offset2grid: normalise to [-1,1] in fp32, then spatial_transformer_sampler maps back (+1 for its zero ring)
  float xc = offx + (float)b + (float)kx;
  float yc = offy + (float)a + (float)ky;
  xc = (xc / (float)(Wp - 1) - 0.5f) * 2.f;
  yc = (yc / (float)(Hp - 1) - 0.5f) * 2.f;
  const float u = (xc + 1.f) * (float)(Wp - 1) / 2.f + 1.f;
  const float v = (yc + 1.f) * (float)(Hp - 1) / 2.f + 1.f;
  const float uc = fminf(fmaxf(u, 0.f), (float)(Wp + 1));
  const float vc = fminf(fmaxf(v, 0.f), (float)(Hp + 1));
  DeformGeom g;
  g.u0 = min(max((int)floorf(uc), 0), Wp);
  g.v0 = min(max((int)floorf(vc), 0), Hp);
  g.wu0 = uc - (float)g.u0;
  g.wu1 = (float)(g.u0 + 1) - uc;
  g.wv0 = vc - (float)g.v0;
  g.wv1 = (float)(g.v0 + 1) - vc;
  g.mu = (u > 0.f) && (u < (float)(Wp + 1));
  g.mv = (v > 0.f) && (v < (float)(Hp + 1));
  return g;
}

// corner (vv,uu) of the doubly padded frame -> offset into the unpadded image or -1
__device__ __forceinline__ int deform_corner(int vv, int uu, int H, int W, int pad) {
  const int y = vv - pad - 1, x = uu - pad - 1;
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? y * W + x : -1;
}

// One sample of the 3 x 3, pad 1 layers: its four corners as offsets into the unpadded plane (-1: outside, in the sampler's zero
// padding), their bilinear weights, and the one-dimensional weights and masks they were made of.
// Corner order: 1 = (v0, u0), 2 = (v0, u0 + 1), 3 = (v0 + 1, u0), 4 = (v0 + 1, u0 + 1).
struct DeformTap {
  DeformGeom g;
  int o1, o2, o3, o4;
  __device__ __forceinline__ float w1() const { return g.wu1 * g.wv1; }
  __device__ __forceinline__ float w2() const { return g.wu0 * g.wv1; }
  __device__ __forceinline__ float w3() const { return g.wu1 * g.wv0; }
  __device__ __forceinline__ float w4() const { return g.wu0 * g.wv0; }
};

// tap (ky, kx) = (t / 3, t % 3) at row a, column b of an H x W plane, displaced by (offx, offy).  (The fused kernels' corner tables pass
// ky and kx themselves: formed at the call, they compile to the instructions those hand-scheduled kernels had before.)
__device__ __forceinline__ DeformTap deform_tap(float offx, float offy, int a, int b, int ky, int kx, int H, int W) {
  DeformTap s;
  s.g = deform_geom(offx, offy, a, b, ky, kx, H, W, 1);
  s.o1 = deform_corner(s.g.v0, s.g.u0, H, W, 1);
  s.o2 = deform_corner(s.g.v0, s.g.u0 + 1, H, W, 1);
  s.o3 = deform_corner(s.g.v0 + 1, s.g.u0, H, W, 1);
  s.o4 = deform_corner(s.g.v0 + 1, s.g.u0 + 1, H, W, 1);
  return s;
}

// the same for position p, the displacement read from one image's offset planes `on` (18 x plane: x offsets of the nine taps, then y)
__device__ __forceinline__ DeformTap deform_tap(const float* __restrict__ on, int t, int p, int H, int W) {
  const int plane = H * W;
  const int a = p / W, b = p - a * W;
  return deform_tap(on[(long)t * plane + p], on[(long)(9 + t) * plane + p], a, b, t / 3, t % 3, H, W);
}

// d sample / d u and d sample / d v of one channel whose values at the four corners are x1 .. x4 (0 outside); wu*, wv*: DeformGeom's
__device__ __forceinline__ float deform_du(float wv0, float wv1, float x1, float x2, float x3, float x4) {
  return -wv1 * x1 + wv1 * x2 - wv0 * x3 + wv0 * x4;
}
__device__ __forceinline__ float deform_dv(float wu0, float wu1, float x1, float x2, float x3, float x4) {
  return -wu1 * x1 - wu0 * x2 + wu1 * x3 + wu0 * x4;
}
__device__ __forceinline__ void deform_coord_grads(const DeformGeom& g, float x1, float x2, float x3, float x4, float& du, float& dv) {
  du = deform_du(g.wv0, g.wv1, x1, x2, x3, x4);
  dv = deform_dv(g.wu0, g.wu1, x1, x2, x3, x4);
}
