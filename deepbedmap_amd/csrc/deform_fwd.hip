// Deformable convolution with the sampler fused into the GEMM (reference srgan_train.py:506-523, :572-574:
// L.DeformableConvolution2D(64 -> 64 | 1, ksize 3, pad 1) on the 4x upsampled planes).
//
// Chainer materialises x_st = the (N, 64*9, H, W) matrix of bilinear samples and multiplies it with W.  At batch 64
// that matrix is 191 MB per layer (3 GB for one 288 x 288 inference crop); deform_sample_kernel + a 1x1 implicit GEMM
// wrote and re-read it.  Here a workgroup samples ONE tap of 64 channels x 64 positions into LDS (16 KB, double
// buffered) and feeds the fp32 MFMAs from there; in a pass nobody differentiates the samples never exist in memory.
//
//   nchw_to_nhwc64_kernel        the layer input once more in channels-last order (what the sampler gathers from)
//   deform_conv64_fused_kernel   64 -> 64 (+ bias, LeakyReLU): MFMA, M = 64 out channels, N = 64 positions, K = 9 x 64
//   deform_conv1_fused_kernel    64 -> 1  (+ bias): a dot product per position, no LDS tile
// (+ the split-bf16 64 -> 64 form and the premultiplied 64 -> 1 form below; the LDS-window forms of the 64 -> 64 layer are in
//  deform_window.hip, the backward kernels in deform_bwd.hip, what they all share in deform_tile.h)
//
// What bounds a sampler is the number of gather INSTRUCTIONS (the texture addresser spends 20-30 cycles on a wave-wide
// dword gather: 3 M of them per layer at batch 64 = the 83 us of deform_sample_kernel, however little they fetch).
// From a channels-last copy the 64 channels of a corner are one contiguous 256-byte run: sixteen lanes fetch it with
// one 16-byte load each, a wave instruction covers four (position, corner) runs, and a tap costs a quarter of the
// instructions, all of them fully coalesced.  The corner offsets and bilinear weights of the tile's 64 positions x 9
// taps are computed once per workgroup into an LDS table (the fp32 normalise / denormalise round trip of Chainer's
// sampler costs two divisions per coordinate).
//
// Roles inside a 256-thread workgroup: SAMPLER -- lane = (position lane >> 4, channel quad lane & 15), wavefront w
// owns positions 16 w .. 16 w + 15 in four steps; MULTIPLIER (64 -> 64) -- wavefront w owns the 32 x 32 output tile
// (channels 32 (w & 1) .., positions 32 (w >> 1) ..) over the whole K.  The gathers of tap t + 1 are issued BEFORE
// the MFMAs of tap t and blended / written to LDS after them.
#include "dbm_internal.h"
#include "kernels.h"
#include "deform_tile.h"
#include "deform_window.h"

namespace {

// x (N, 64, plane) -> xt (N * plane, 64)
__global__ __launch_bounds__(256) void nchw_to_nhwc64_kernel(const float* __restrict__ x, float* __restrict__ xt, long total, int plane) {
  __shared__ float tile[64 * DF_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long P0 = (long)blockIdx.x * 64;
  {
    const long P = P0 + lane;
    if (P < total) {
      const long n = P / plane;
      const float* src = x + (n * 64) * plane + (P - n * plane);
#pragma unroll
      for (int i = 0; i < 16; ++i) tile[(16 * wave + i) * DF_LD + lane] = src[(long)(16 * wave + i) * plane];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long P = P0 + 16 * wave + i;
    if (P < total) xt[P * 64 + lane] = tile[lane * DF_LD + 16 * wave + i];
  }
}

// y (N, 64, plane) = act(bias + W * samples); yt (optional): the same output channels-last (the next deformable layer's
// sampler input); colout (optional): the samples, (N, 576, plane) with row c * 9 + t (a retained pass: the weight
// gradient reads them).
__global__ __launch_bounds__(256) void deform_conv64_fused_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                  const float* __restrict__ wf, const float* __restrict__ bias,
                                                                  float* __restrict__ y, float* __restrict__ yt,
                                                                  float* __restrict__ colout, int N, int H, int W, long offsn, int act,
                                                                  float slope, int abl) {
  __shared__ TileGeometry geo;
  __shared__ float col[2][64 * DF_LD];  // [buffer][channel][position]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const long P0 = (long)blockIdx.x * DF_POS;
  build_geometry(geo, off, offsn, P0, total, plane, H, W, tid, abl);
  // ---- sampler role ----
  const int q = lane & 15, pi = lane >> 4;
  const float* xq = xt + 4 * q;
  // ---- multiplier role ----
  const int ct = wave & 1, pt = wave >> 1, j = lane & 31, kh = lane >> 5;
  const float* wl = wf + (long)kh * 9 * 64 + ct * 32 + j;  // + ((2 cp) * 9 + t) * 64
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  __syncthreads();

  CornerRequest cr;
  auto gather = [&](int t) { cr.request(geo, xq, t, wave, pi); };
  auto blend = [&](float* dst) { cr.write_samples(dst, q, wave, pi); };
  auto spill = [&](int t, const float* src) {  // the tap's samples to the column matrix: 256-byte runs along the positions
    const long P = P0 + lane;
    if (P >= total) return;
    const long n = P / plane;
    float* dst = colout + (n * 576 + t) * plane + (P - n * plane);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = 16 * wave + i;
      dst[(long)c * 9 * plane] = src[c * DF_LD + lane];
    }
  };
  gather(0);
  blend(col[0]);
  __syncthreads();
  auto multiply = [&](int t, bool more) {
    // this tap's weights first, then the next tap's gathers: loads return in order, so the MFMAs wait for the (L2-hot,
    // coalesced) weights only and the gathers stay in flight underneath them.  (`more` is a compile-time constant at
    // both call sites: a branch around the gathers would make the waitcnt bookkeeping at its join assume the worst.)
    float av[32];
#pragma unroll
    for (int cp = 0; cp < 32; ++cp) av[cp] = wl[(long)(cp * 18 + t) * 64];
    __builtin_amdgcn_sched_barrier(0);
    if (more) gather(t + 1);
    __builtin_amdgcn_sched_barrier(0);  // the requests above stay in front of the MFMA block they overlap
    const float* cb = col[t & 1] + kh * DF_LD + pt * 32 + j;
#pragma unroll
    for (int cp = 0; cp < 32; ++cp) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cp], cb[cp * 2 * DF_LD], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (colout) spill(t, col[t & 1]);
    if (more) blend(col[(t + 1) & 1]);
    __syncthreads();
  };
  for (int t = 0; t < 8; ++t) multiply(t, true);
  multiply(8, false);
  // ---- epilogue: bias, LeakyReLU; 128-byte runs along the position axis (+ 16-byte channel quads, channels-last) ----
  const long Pm = P0 + pt * 32 + j;
  if (Pm >= total) return;
  const long nm = Pm / plane;
  float* yn = y + nm * 64 * plane + (Pm - nm * plane);
  float v[16];   // (all bias loads before the first store: see DF_EPILOGUE64_VALUES)
  DF_EPILOGUE64_VALUES(v, acc, ct, kh, bias, act, slope)
  if (y) {
    DF_EPILOGUE64_STORE_Y(v, ct, kh, yn, 0, plane)
  }
  if (yt) {
    DF_EPILOGUE64_STORE_YT(v, ct, kh, yt + Pm * 64)
  }
}

// y (N, 1, plane) = bias + sum_{c,t} w[c*9+t] * sample: lane (position, channel quad) accumulates its four channels over the
// nine taps, the sixteen quads of a position fold with a fixed xor tree.
__global__ __launch_bounds__(256) void deform_conv1_fused_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ y, int N, int H, int W, long offsn, int oc,
                                                                 int co) {
  // (oc > 1: GeneratorModel(out_channels=oc), forward only -- one launch per output channel co, w / bias already offset)
  __shared__ TileGeometry geo;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const long P0 = (long)blockIdx.x * DF_POS;
  build_geometry(geo, off, offsn, P0, total, plane, H, W, tid);
  const int q = lane & 15, pi = lane >> 4;
  const float* xq = xt + 4 * q;
  __shared__ __attribute__((aligned(16))) float wsh[9 * 64];  // [tap][channel]
  for (int e = tid; e < 576; e += 256) wsh[(e % 9) * 64 + e / 9] = w[e];
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    // (its own copy of CornerRequest::request / blended, deform_tile.h: through the struct the two hoisted LDS addresses of this loop
    //  are computed in the other order -- the same instructions in other registers)
    float4 c1[4], c2[4], c3[4], c4[4], cw[4];
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
    const float4 wr = *reinterpret_cast<const float4*>(wsh + t * 64 + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = blend4(cw[i], c1[i], c2[i], c3[i], c4[i]);
      acc[i] = fmaf(wr.x, v.x, acc[i]);
      acc[i] = fmaf(wr.y, v.y, acc[i]);
      acc[i] = fmaf(wr.z, v.z, acc[i]);
      acc[i] = fmaf(wr.w, v.w, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = acc[i];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    const long P = P0 + 16 * wave + 4 * i + pi;
    if (q == 0 && P < total) {
      const long n = P / plane;
      y[(n * oc + co) * plane + (P - n * plane)] = v + (bias ? bias[0] : 0.f);
    }
  }
}

// ---- 64 -> 64 in split-bf16 arithmetic (the bf16 sweep, forward only) ----
// The same sampler; the blended samples are split x = hi + lo (hi = bf16(x), lo = bf16(x - hi)) on their way into LDS and
// the product is three v_mfma_f32_32x32x16_bf16 -- hi*hi + hi*lo + lo*hi, fp32 accumulation, 2^-16 operand precision (the
// arithmetic of conv_cl16x3_kernel, conv_cl16.hip) -- instead of 32 fp32 MFMAs per tap: 384 instead of 2048 matrix-pipe
// cycles per tap and wavefront.  What remains is the sampler's gathers (the 64 -> 1 layer's time before it was re-associated).
//   LDS sample tile: [position][64 channels] bf16, one 128-byte row per position for hi and one for lo, rows 144 bytes apart
//   (any sixteen consecutive rows -- and the lane groups of a ds_read_b128 -- then fall on distinct banks);
//   weights: wx [tap][k step][hi | lo][channel tile][lane][8] bf16 (launch_pack_deform_x3): lane = (out channel lane & 31,
//   k group lane >> 5), one coalesced 16-byte load per fragment.
constexpr int DX_ROW = 144;                 // bytes between positions of the split sample tile
constexpr int DX_TILE = 64 * DX_ROW;        // one (hi or lo) tile

__global__ __launch_bounds__(256) void deform_conv64_x3_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                               const dbf16x8* __restrict__ wx, const float* __restrict__ bias,
                                                               float* __restrict__ y, float* __restrict__ yt, int N, int H, int W,
                                                               long offsn, int act, float slope) {
  __shared__ TileGeometry geo;
  __shared__ __attribute__((aligned(16))) unsigned char col[2][2 * DX_TILE];  // [buffer][hi | lo][position][64 bf16 (+ pad)]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const long P0 = (long)blockIdx.x * DF_POS;
  build_geometry(geo, off, offsn, P0, total, plane, H, W, tid);
  const int q = lane & 15, pi = lane >> 4;            // sampler role
  const float* xq = xt + 4 * q;
  const int ct = wave & 1, pt = wave >> 1, j = lane & 31, kg = lane >> 5;   // multiplier role
  const dbf16x8* wl = wx + ct * 64 + lane;            // + ((t * 4 + ks) * 2 + hl) * 128
  const int boff = (pt * 32 + j) * DX_ROW + kg * 16;  // + ks * 32 (+ DX_TILE for lo)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  __syncthreads();

  CornerRequest cr;
  auto gather = [&](int t) { cr.request(geo, xq, t, wave, pi); };
  auto blend = [&](unsigned char* dst) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = cr.blended(i);
      const float f[4] = {v.x, v.y, v.z, v.w};
      dbf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        hi[e] = (__bf16)f[e];
        lo[e] = (__bf16)(f[e] - (float)hi[e]);
      }
      unsigned char* d = dst + (16 * wave + 4 * i + pi) * DX_ROW + 8 * q;
      *reinterpret_cast<dbf16x4*>(d) = hi;
      *reinterpret_cast<dbf16x4*>(d + DX_TILE) = lo;
    }
  };
  gather(0);
  blend(col[0]);
  __syncthreads();
  auto multiply = [&](int t, bool more) {
    dbf16x8 ah[4], al[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      ah[ks] = wl[((t * 4 + ks) * 2 + 0) * 128];
      al[ks] = wl[((t * 4 + ks) * 2 + 1) * 128];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) gather(t + 1);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char* cb = col[t & 1] + boff;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const dbf16x8 bh = *reinterpret_cast<const dbf16x8*>(cb + ks * 32);
      const dbf16x8 bl = *reinterpret_cast<const dbf16x8*>(cb + ks * 32 + DX_TILE);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks], bl, acc, 0, 0, 0);   // small terms first
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ks], bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks], bh, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) blend(col[(t + 1) & 1]);
    __syncthreads();
  };
  for (int t = 0; t < 8; ++t) multiply(t, true);
  multiply(8, false);
  const long Pm = P0 + pt * 32 + j;
  if (Pm >= total) return;
  const long nm = Pm / plane;
  float v[16];   // (all bias loads before the first store: see DF_EPILOGUE64_VALUES)
  DF_EPILOGUE64_VALUES(v, acc, ct, kg, bias, act, slope)
  if (y) {
    DF_EPILOGUE64_STORE_Y(v, ct, kg, y, nm * 64 * plane + (Pm - nm * plane), plane)
  }
  if (yt) {
    DF_EPILOGUE64_STORE_YT(v, ct, kg, yt + Pm * 64)
  }
}

// w: canonical OIHW (64, 64, 3, 3) -> wx [tap][k step][hi | lo][channel tile][lane][8]
__global__ __launch_bounds__(256) void pack_deform_x3_kernel(const float* __restrict__ w, __bf16* __restrict__ wx) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // (t, ks, ct, lane, e)
  if (idx >= 9 * 4 * 2 * 64 * 8) return;
  const int e = idx & 7, lane = (idx >> 3) & 63, ct = (idx >> 9) & 1, ks = (idx >> 10) & 3, t = idx >> 12;
  const int o = ct * 32 + (lane & 31), c = 16 * ks + 8 * (lane >> 5) + e;
  const float v = w[((long)o * 64 + c) * 9 + t];
  const __bf16 hi = (__bf16)v;
  const __bf16 lo = (__bf16)(v - (float)hi);
  const long base = ((long)(t * 4 + ks) * 2) * 1024 + (ct * 64 + lane) * 8 + e;
  wx[base] = hi;
  wx[base + 1024] = lo;
}

// ---- the few-output-channel layer (64 -> 1: the DEM itself) with the multiplication BEFORE the sampler ----
// Bilinear sampling is linear in the sampled plane: sum_c w[c][t] * sample(x_c, pos) = sample(sum_c w[c][t] * x_c, pos).  So the
// layer is a 1x1 convolution 64 -> 9 (one plane z_t per tap, deform1_premul_kernel: reads the input once, coalesced) followed by
// nine four-corner gathers of single floats per position (deform1_sample_kernel) -- instead of gathering 9 x 4 x 256 bytes per
// position through the vector L1 (deform_conv1_fused_kernel: 12 GB of gathers for one 1144 x 1144 plane, 0.65 ms; now 0.34 + 0.05 GB).
// The sums are associated differently (channels first, then corners and taps), i.e. equal to the other order to fp32 rounding.
//
// z[(n * nz + k) * plane + p] = sum_c w[k * 64 + c'] ..., k = co * 9 + t, w in its canonical OIHW order (co, c, t)
__global__ __launch_bounds__(256) void deform1_premul_kernel(const float* __restrict__ xt, const float* __restrict__ w, float* __restrict__ z,
                                                             long total, int plane, int nz) {
  extern __shared__ __attribute__((aligned(16))) float pm[];  // wsh[nz][64] | zt[nz][64]
  float* wsh = pm;
  float* zt = pm + nz * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < nz * 64; e += 256) {  // e = k * 64 + c  <-  w[(co * 64 + c) * 9 + t]
    const int k = e >> 6, c = e & 63, co = k / 9, t = k - 9 * co;
    wsh[e] = w[((long)co * 64 + c) * 9 + t];
  }
  __syncthreads();
  const int q = lane & 15, pi = lane >> 4;
  const long P0 = (long)blockIdx.x * 64;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pl = 16 * wave + 4 * i + pi;
    const long P = P0 + pl;
    const float4 v = P < total ? *reinterpret_cast<const float4*>(xt + P * 64 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < nz; ++k) {
      const float4 wr = *reinterpret_cast<const float4*>(wsh + k * 64 + 4 * q);
      float a = wr.x * v.x;
      a = fmaf(wr.y, v.y, a);
      a = fmaf(wr.z, v.z, a);
      a = fmaf(wr.w, v.w, a);
      a += __shfl_xor(a, 1, 64);
      a += __shfl_xor(a, 2, 64);
      a += __shfl_xor(a, 4, 64);
      a += __shfl_xor(a, 8, 64);
      if (q == 0) zt[k * 64 + pl] = a;
    }
  }
  __syncthreads();
  const long P = P0 + lane;
  if (P < total) {
    const long n = P / plane;
    float* dst = z + n * nz * plane + (P - n * plane);
    for (int k = wave; k < nz; k += 4) dst[(long)k * plane] = zt[k * 64 + lane];
  }
}

// The same premultiplication on the matrix pipes (round 6; nz <= 16, i.e. the model's own 64 -> 1 layer): the kernel above spends four
// FMAs, four cross-lane adds and an LDS write per (position, tap) on sixteen lanes -- 180 of the 220 us of the layer on a 1144 x 1144
// plane, against 42 us for reading the plane once.  Here z (16 rows, nz live) x 16 positions = W (16 x 64) . x (64 x 16 positions) is
// sixteen v_mfma_f32_16x16x4f32 per wavefront and 16 positions: lane (j, kq) holds row j of W for the channels kq * 16 .. + 15 (registers,
// loaded once) and reads those sixteen channels of position j as ONE 64-byte run; step s multiplies the channels {kq * 16 + s}.  fp32
// operands, fp32 accumulation; the channels are summed in another order than above (equal to fp32 rounding).
typedef float f32x4m __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void deform1_premul_mfma_kernel(const float* __restrict__ xt, const float* __restrict__ w,
                                                                  float* __restrict__ z, int total, int plane, int nz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, kq = lane >> 4;
  float a[16];
  {
    const int co = j / 9, t = j - 9 * co;   // row j of z = (output channel co, tap t); w in its canonical OIHW order (co, c, t)
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = j < nz ? w[((long)co * 64 + kq * 16 + s) * 9 + t] : 0.f;
  }
  // A tile's 16 positions x 64 channels = 4 KB, contiguous in memory: four coalesced 1 KB loads per wavefront (lane -> 16 consecutive
  // bytes), transposed into the MFMA's B layout through a private LDS tile (rows of 272 bytes: conflict-free both ways).  Reading the
  // B layout straight from memory -- lane (j, kq) = 64 bytes at position j, sixteen such lanes 256 bytes apart -- touched 64 cache
  // lines per load instruction.
  __shared__ __attribute__((aligned(16))) float tl[4][16 * 68];
  float* mine = tl[wave];
  const long nfl = (long)total * 64;
  const int ntile = (total + 15) >> 4;
  for (int tile = blockIdx.x * 4 + wave; tile < ntile; tile += gridDim.x * 4) {
    const int P = tile * 16 + j;
    float4 g[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const long idx = (long)tile * 1024 + m * 256 + lane * 4;
      g[m] = idx < nfl ? *reinterpret_cast<const float4*>(xt + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) *reinterpret_cast<float4*>(mine + (4 * m + (lane >> 4)) * 68 + (lane & 15) * 4) = g[m];
    float4 b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) b[m] = *reinterpret_cast<const float4*>(mine + j * 68 + kq * 16 + 4 * m);
    f32x4m acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * m + 0], b[m].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * m + 1], b[m].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * m + 2], b[m].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * m + 3], b[m].w, acc, 0, 0, 0);
    }
    if (P < total) {   // lane (j, kq) holds rows 4 kq .. 4 kq + 3 of column j
      const int n = P / plane, p = P - n * plane;
      float* dst = z + ((long)n * nz + 4 * kq) * plane + p;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * kq + r < nz) dst[(long)r * plane] = acc[r];
    }
  }
}

static void launch_premul(const float* xt, const float* w, float* z, long total, int plane, int nz, hipStream_t s) {
  // (planes of the sweep only: on the training tile's 83 k positions the two kernels take the same time inside the iteration, and the
  //  discriminator's theoretically-zero linear_2/b gradient -- rounding noise of 128 cancelling terms, held to 3.2e-7 by
  //  tests/test_gpu_dem.py -- moves with the last bit of any fake: the training path keeps the summation order it was pinned with)
  if (nz <= 16 && total >= (1L << 18) && total < (1L << 31)) {
    const long ntile = (total + 15) / 16;
    const unsigned blocks = (unsigned)std::min<long>((ntile + 3) / 4, 4096);
    hipLaunchKernelGGL(deform1_premul_mfma_kernel, dim3(blocks), dim3(256), 0, s, xt, w, z, (int)total, plane, nz);
    return;
  }
  static bool attr = false;   // (O >= 15: 2 * 9 * O * 64 floats exceed the 64 KB default of dynamic LDS)
  if (!attr) {
    DBM_HIP(hipFuncSetAttribute((const void*)deform1_premul_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 9 * 16 * 64 * (int)sizeof(float)));
    attr = true;
  }
  const unsigned blocks = (unsigned)((total + DF_POS - 1) / DF_POS);
  hipLaunchKernelGGL(deform1_premul_kernel, dim3(blocks), dim3(256), (size_t)2 * nz * 64 * sizeof(float), s, xt, w, z, total, plane, nz);
}

// y[(n * oc + co) * plane + p] = bias[co] + sum_t bilinear(z[n][co * 9 + t], p + tap_t + offset_t(p));  blockIdx.y = co
__global__ __launch_bounds__(256) void deform1_sample_kernel(const float* __restrict__ z, const float* __restrict__ off,
                                                             const float* __restrict__ bias, float* __restrict__ y, long total, int H, int W,
                                                             long offsn, int oc) {
  const long P = (long)blockIdx.x * 256 + threadIdx.x;
  if (P >= total) return;
  const int plane = H * W, co = blockIdx.y;
  const int n = (int)(P / plane);
  const int p = (int)(P - (long)n * plane);
  const int a = p / W, b = p - a * W;
  const float* on = off + (long)n * offsn + p;
  const float* zn = z + ((long)n * oc + co) * 9 * plane;
  float ox[9], oy[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) { ox[t] = on[(long)t * plane]; oy[t] = on[(long)(9 + t) * plane]; }
  float acc = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const DeformGeom g = deform_geom(ox[t], oy[t], a, b, t / 3, t % 3, H, W, 1);
    const int o1 = deform_corner(g.v0, g.u0, H, W, 1), o2 = deform_corner(g.v0, g.u0 + 1, H, W, 1);
    const int o3 = deform_corner(g.v0 + 1, g.u0, H, W, 1), o4 = deform_corner(g.v0 + 1, g.u0 + 1, H, W, 1);
    const float* zt = zn + (long)t * plane;
    const float z1 = zt[o1 >= 0 ? o1 : 0], z2 = zt[o2 >= 0 ? o2 : 0], z3 = zt[o3 >= 0 ? o3 : 0], z4 = zt[o4 >= 0 ? o4 : 0];
    float v = (o1 >= 0 ? g.wu1 * g.wv1 : 0.f) * z1;
    v = fmaf(o2 >= 0 ? g.wu0 * g.wv1 : 0.f, z2, v);
    v = fmaf(o3 >= 0 ? g.wu1 * g.wv0 : 0.f, z3, v);
    v = fmaf(o4 >= 0 ? g.wu0 * g.wv0 : 0.f, z4, v);
    acc += v;
  }
  y[((long)n * oc + co) * plane + p] = acc + (bias ? bias[co] : 0.f);
}

}  // namespace

bool deform_conv_fused_ok(int C, int O) { return C == 64 && (O == 64 || (O >= 1 && O <= 16)); }

void launch_nchw_to_nhwc64(const float* x, float* xt, int N, int plane, hipStream_t s) {
  const long total = (long)N * plane;
  hipLaunchKernelGGL(nchw_to_nhwc64_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, s, x, xt, total, plane);
  DBM_HIP(hipGetLastError());
}

// xt: the layer input channels-last (launch_nchw_to_nhwc64, or the previous fused layer's `yt`).
// O == 64: w = the packed forward image [576][64] of the layer viewed as a 1x1 convolution over (c, tap) columns
// (IgLayer::wf, k = c * 9 + t); O == 1: w = the canonical (1, 64, 3, 3) tensor.  y (N, O, H, W) is overwritten.
// O <= 16 with a scratch `z` of N * 9 * O * H * W floats: the premultiplied form (deform1_premul_kernel + deform1_sample_kernel);
// z == nullptr: the gather-then-multiply kernel.  O == 64: y may be null when only the channels-last output yt is wanted.
void launch_deform_conv_fused(const float* xt, const float* off, const float* w, const float* bias, float* y, float* yt, float* colout,
                              int N, int C, int H, int W, long offsn, int O, int act, float slope, hipStream_t s, float* z) {
  DBM_CHECK(deform_conv_fused_ok(C, O), "fused deformable convolution: 64 input channels, 64 or <= 16 output channels");
  const long total = (long)N * H * W;
  DBM_CHECK(total < (1L << 31), "fused deformable convolution: more than 2^31 positions");
  // (the window form: planes narrow enough that <= 128 consecutive positions + their vertical reach fit the LDS layout, no sample matrix
  //  wanted -- the same bits as the gathering kernel.  119-125 against 111 us standalone on the training tile (one workgroup of four
  //  wavefronts per CU; 704 tiles = three rounds), but 7.56-7.58 against 7.59-7.61 ms per step in three A/B series: it leaves the CUs to
  //  the kernels of the other streams.  DBM_DEFORM_FWD_WINDOW=0: the gathering kernel.  profiles/r6/ab_deform_fwd_fp32_window.txt)
  static const int fwin_env = getenv("DBM_DEFORM_FWD_WINDOW") ? atoi(getenv("DBM_DEFORM_FWD_WINDOW")) : 1;
  const int span_rows = std::min(H, (DWF_POS - 1 + W - 1) / W + 1);   // most rows 128 consecutive positions can span
  const bool fwin_ok = O == 64 && !colout && fwin_env && (span_rows + 2 * DWF_R + 3) * (W + 2 * DWF_R + 3) <= DWF_MAXPIX &&
                       deform_window_plane_ok(H, W);
  const unsigned blocks = (unsigned)((total + DF_POS - 1) / DF_POS);
  if (g_profiler.enabled) {
    // algorithmic bytes: the NHWC input and the 18 offset planes once, the weights once, the output (and its NHWC twin / the
    // kept sampled columns of a training forward) once
    const double bytes = 4.0 * ((double)total * (C + 18 + (y ? O : 0) + (yt ? O : 0) + (colout ? 9.0 * C : 0.0)) + 9.0 * C * O);
    char tag[40];
    snprintf(tag, sizeof(tag), "deform%d%s_%dx%d_n%d%s", O, fwin_ok ? "w" : "", H, W, N, colout ? "_keep" : "");
    g_profiler.begin(s, 0, 2.0 * (double)total * O * C * 9, bytes, tag, blocks);
  }
  if (fwin_ok)
    launch_deform_conv64_fusedw(xt, off, w, bias, y, yt, N, H, W, offsn, act, slope, s);
  else if (O == 64)
    hipLaunchKernelGGL(deform_conv64_fused_kernel, dim3(blocks), dim3(256), 0, s, xt, off, w, bias, y, yt, colout, N, H, W, offsn, act, slope,
                       DBM_MEASURE_ENV("DEFORM_ABL"));
  else if (z) {
    const int nz = 9 * O;
    launch_premul(xt, w, z, total, H * W, nz, s);
    hipLaunchKernelGGL(deform1_sample_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)O), dim3(256), 0, s, z, off, bias, y, total, H, W,
                       offsn, O);
  } else
    for (int co = 0; co < O; ++co)  // (w: OIHW (O, 64, 3, 3))
      hipLaunchKernelGGL(deform_conv1_fused_kernel, dim3(blocks), dim3(256), 0, s, xt, off, w + (long)co * 576, bias ? bias + co : nullptr,
                         y, N, H, W, offsn, O, co);
  if (g_profiler.enabled) g_profiler.end(s);
  DBM_HIP(hipGetLastError());
}

size_t deform_x3_packed_elems() { return (size_t)9 * 4 * 2 * 2 * 64 * 8; }
void launch_pack_deform_x3(const float* w_oihw, void* dst, hipStream_t s) {
  hipLaunchKernelGGL(pack_deform_x3_kernel, dim3((9 * 4 * 2 * 64 * 8 + 255) / 256), dim3(256), 0, s, w_oihw, (__bf16*)dst);
  DBM_HIP(hipGetLastError());
}
// the 64 -> 64 layer in split-bf16 arithmetic (forward only): wx from launch_pack_deform_x3; y and / or yt
// window: 0 the gathering kernel, 1 the LDS-window kernel, -1 the launcher's choice (DBM_DEFORM_X3_WINDOW, default: the window on planes
// with at least one workgroup per CU)
void launch_deform_conv64_x3(const float* xt, const float* off, const void* wx, const float* bias, float* y, float* yt, int N, int H, int W,
                             long offsn, int act, float slope, hipStream_t s, int window) {
  const long total = (long)N * H * W;
  DBM_CHECK(total < (1L << 31), "fused deformable convolution: more than 2^31 positions");
  const int tilesX = (W + DW_T - 1) / DW_T, tilesY = (H + DW_T - 1) / DW_T;
  const long tiles = (long)N * tilesX * tilesY;
  const bool plane_ok = deform_window_plane_ok(H, W);
  if (window < 0) {
    static const int env = getenv("DBM_DEFORM_X3_WINDOW") ? atoi(getenv("DBM_DEFORM_X3_WINDOW")) : 1;
    window = env && tiles >= 256 && plane_ok ? 1 : 0;
  } else if (window) {
    DBM_CHECK(plane_ok, "deformable convolution, LDS-window kernel: the plane exceeds its limits (" DBM_DEFORM_WINDOW_LIMITS ")");
  }
  const unsigned blocks = window ? (unsigned)tiles : (unsigned)((total + DF_POS - 1) / DF_POS);
  if (g_profiler.enabled) {
    const double bytes = 4.0 * (double)total * (64 + 18 + (y ? 64 : 0) + (yt ? 64 : 0)) + 2.0 * 2.0 * 9 * 64 * 64;
    char tag[40];
    snprintf(tag, sizeof(tag), "deform64x3%s_%dx%d_n%d", window ? "w" : "", H, W, N);
    g_profiler.begin(s, 0, 2.0 * (double)total * 64 * 64 * 9, bytes, tag, blocks);
  }
  if (window)
    launch_deform_conv64_x3w(xt, off, wx, bias, y, yt, N, H, W, offsn, act, slope, tilesX, tilesY, s);
  else
    hipLaunchKernelGGL(deform_conv64_x3_kernel, dim3(blocks), dim3(256), 0, s, xt, off, (const dbf16x8*)wx, bias, y, yt, N, H, W, offsn, act,
                       slope);
  if (g_profiler.enabled) g_profiler.end(s);
  DBM_HIP(hipGetLastError());
}

// z[n][t][p] = sum_c w[c][t] x_c(p) for the O == 1 layer (the forward's premultiplication alone: the op-level backward entry point)
void launch_deform1_premul(const float* xt, const float* w, float* z, int N, int H, int W, int O, hipStream_t s) {
  const long total = (long)N * H * W;
  DBM_CHECK(O >= 1 && O <= 16, "launch_deform1_premul: up to sixteen output channels");
  launch_premul(xt, w, z, total, H * W, 9 * O, s);
  DBM_HIP(hipGetLastError());
}
