// Non-GEMM kernels of the hot path: few-input-channel convolutions (input block, D conv0), im2col,
// 2x2 sum-pool (backward of the nearest upsample), row gather.  All are HBM/L2-bound VALU kernels:
// one position per lane, coalesced along the innermost (x) axis of the NCHW fp32 tensors.
#include "dbm_internal.h"
#include "kernels.h"
#include <cstdlib>

// ----------------------------------------------------------------------------------------------
// Convolution with 1 or 2 input channels (reference srgan_train.py:223-254 input block, :617-625
// discriminator conv_layer0).  Each thread owns one output position and 8 output channels.
// ----------------------------------------------------------------------------------------------
// K3: 3x3 kernels (the discriminator's conv_layer0, the input block's 3x3 branches) with the tap loops unrolled and branch-free -- every
// input value and every weight of a channel requested together (the general form's run-time loops with their `continue` made nine
// dependent round trips of a 1-channel 3x3 layer: 14.8 us for a 21 MB output).
template <bool K3>
__global__ __launch_bounds__(256) void smallcin_conv_fwd_kernel(const SmallConvDesc d) {
  const int plane = d.OH * d.OW;
  const long P = (long)blockIdx.x * 64 + (threadIdx.x & 63);
  const int cg = threadIdx.x >> 6;  // wave-uniform: 8-channel group within the 32 handled per block
  const int co0 = blockIdx.y * 32 + cg * 8;
  if (P >= (long)d.N * plane || co0 >= d.Cout) return;
  const int n = (int)(P / plane);
  const int r = (int)(P - (long)n * plane);
  const int a = r / d.OW, b = r - a * d.OW;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = d.bias ? d.bias[co0 + i] : 0.f;
  const int K = d.Cin * d.KH * d.KW;
  if (K3) {
    for (int c = 0; c < d.Cin; ++c) {
      const float* xc = d.x + (long)n * d.xsn + (long)c * d.Hin * d.Win;
      float xv[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int iy = a * d.stride - d.pad + t / 3, ix = b * d.stride - d.pad + t % 3;
        const bool in = (unsigned)iy < (unsigned)d.Hin && (unsigned)ix < (unsigned)d.Win;
        const float v = xc[in ? (long)iy * d.Win + ix : 0];
        xv[t] = in ? v : 0.f;
      }
      const float* wr = d.w + (long)co0 * K + c * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t)   // (tap order ky, kx as in the general form: the same sums)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(wr[(long)i * K + t], xv[t], acc[i]);
    }
  } else
  for (int c = 0; c < d.Cin; ++c) {
    const float* xc = d.x + (long)n * d.xsn + (long)c * d.Hin * d.Win;
    for (int ky = 0; ky < d.KH; ++ky) {
      const int iy = a * d.stride - d.pad + ky;
      if ((unsigned)iy >= (unsigned)d.Hin) continue;
      const float* xr = xc + (long)iy * d.Win;
      const float* wr = d.w + (long)co0 * K + (c * d.KH + ky) * d.KW;
      for (int kx = 0; kx < d.KW; ++kx) {
        const int ix = b * d.stride - d.pad + kx;
        const float v = ((unsigned)ix < (unsigned)d.Win) ? xr[ix] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(wr[(long)i * K + kx], v, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float v = acc[i];
    if (d.act) v = v >= 0.f ? v : d.slope * v;
    d.y[(long)n * d.ysn + (long)(co0 + i) * plane + r] = v;
  }
}

void launch_smallcin_conv_fwd(const SmallConvDesc& d, hipStream_t s) {
  if (dbm_abl_skip() & 128) return;  // (libdbm_measure.so only)
  DBM_CHECK(d.Cout % 8 == 0, "smallcin conv: Cout must be a multiple of 8");
  const long total = (long)d.N * d.OH * d.OW;
  dim3 grid((unsigned)((total + 63) / 64), (unsigned)((d.Cout + 31) / 32));
  if (d.KH == 3 && d.KW == 3) hipLaunchKernelGGL(smallcin_conv_fwd_kernel<true>, grid, dim3(256), 0, s, d);
  else hipLaunchKernelGGL(smallcin_conv_fwd_kernel<false>, grid, dim3(256), 0, s, d);
  DBM_HIP(hipGetLastError());
}

// gW[o][c][ky][kx] += sum_{n,a,b} dy[n][o][a][b] * x[n][c][a*s-p+ky][b*s-p+kx];  gb[o] += sum dy.
// One WORKGROUP per weight element (and one per bias element): its 256 threads stride over the output positions
// and the partial sums are folded by a fixed shuffle / LDS tree -- no K split across workgroups, so the one atomic
// per element only orders separate launches (the two graphs of the discriminator: a + b == b + a).  Reproducible.
__global__ __launch_bounds__(256) void smallcin_conv_wgrad_kernel(const SmallConvDesc d, const float* __restrict__ dy,
                                                                  long dysn, float* gW, float* gb) {
  __shared__ float sh[4];
  const int K = d.Cin * d.KH * d.KW;
  const int e = blockIdx.x;
  const int plane = d.OH * d.OW;
  const bool bias = e >= d.Cout * K;
  const int o = bias ? e - d.Cout * K : e / K;
  const int k = bias ? 0 : e - o * K;
  const int c = k / (d.KH * d.KW), kr = k - c * d.KH * d.KW;
  const int ky = kr / d.KW, kx = kr - ky * d.KW;
  // lanes run along the flattened (n, a, b) positions: coalesced dy reads; two multiply-high divisions per element
  const unsigned total = (unsigned)d.N * (unsigned)plane;
  const unsigned planeM = 0xffffffffu / (unsigned)plane, owM = 0xffffffffu / (unsigned)d.OW;  // floor((2^32-1)/d): <= 1 short
  float acc = 0.f;
  // (eight positions per thread and trip, all sixteen loads requested before the first multiply-add: the one-position form was twenty
  //  dependent pairs of round trips per thread -- 14.5 us, twice, at the very end of a training iteration.  Same order of sums.)
  for (unsigned P0 = threadIdx.x; P0 < total; P0 += 256 * 8) {
    float g[8], xv[8];
    bool use[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned Pu = P0 + 256u * (unsigned)u;
      const bool in = Pu < total;
      const unsigned P = in ? Pu : 0u;
      unsigned n = __umulhi(P, planeM);
      unsigned r = P - n * (unsigned)plane;
      if (r >= (unsigned)plane) { ++n; r -= (unsigned)plane; }
      g[u] = dy[(long)n * dysn + (long)o * plane + r];
      unsigned a = __umulhi(r, owM);
      unsigned b = r - a * (unsigned)d.OW;
      if (b >= (unsigned)d.OW) { ++a; b -= (unsigned)d.OW; }
      const int iy = (int)a * d.stride - d.pad + ky, ix = (int)b * d.stride - d.pad + kx;
      const bool inside = !bias && (unsigned)iy < (unsigned)d.Hin && (unsigned)ix < (unsigned)d.Win;
      xv[u] = d.x[inside ? (long)n * d.xsn + (long)c * d.Hin * d.Win + (long)iy * d.Win + ix : 0];
      use[u] = in && (bias || inside);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float t = bias ? acc + g[u] : fmaf(g[u], xv[u], acc);
      acc = use[u] ? t : acc;
    }
  }
  for (int s2 = 32; s2 > 0; s2 >>= 1) acc += __shfl_down(acc, s2, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if (bias) atomicAdd(gb + o, v);
    else atomicAdd(gW + e, v);
  }
}

// conv_layer0 of the discriminator (one input channel, 3 x 3, stride 1, pad 1): a workgroup per (output channel group, position
// slice) keeps all nine sums and the bias sum in registers, so dy is read ONCE instead of ten times; the slices' partial sums go to
// a scratch buffer and a second kernel adds them in slice order (reproducible like the kernel above; 249 -> ~30 us).
constexpr int SCW_SLICES = 64;
constexpr int SCW_OG = 8;  // output channels per workgroup
// The geometry is known at compile time: with (c, ky, kx) decoded per tap by runtime integer divisions a position cost ~600 VALU
// instructions against ten FMAs.  SCW_OG output channels per workgroup (blockIdx.x = channel group): a position's nine input
// values are loaded once for all of them (the loads of x, not of dy, were the bulk of the instructions: 49 -> ~15 us).
__global__ __launch_bounds__(256) void smallcin_wgrad_partial_kernel(const SmallConvDesc d, const float* __restrict__ dy,
                                                                     long dysn, float* __restrict__ partial) {
  constexpr int OG = SCW_OG;
  __shared__ float sh[4][OG * 10];
  const int o0 = blockIdx.x * OG, z = blockIdx.y;
  const int plane = d.OH * d.OW;
  const unsigned total = (unsigned)d.N * (unsigned)plane;
  const unsigned chunk = (total + SCW_SLICES - 1) / SCW_SLICES;
  const unsigned p0 = z * chunk, p1 = min(total, p0 + chunk);
  const unsigned planeM = 0xffffffffu / (unsigned)plane, owM = 0xffffffffu / (unsigned)d.OW;
  float acc[OG][10];
#pragma unroll
  for (int oo = 0; oo < OG; ++oo)
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[oo][k] = 0.f;
  for (unsigned P = p0 + threadIdx.x; P < p1; P += 256) {
    unsigned n = __umulhi(P, planeM);
    unsigned r = P - n * (unsigned)plane;
    if (r >= (unsigned)plane) { ++n; r -= (unsigned)plane; }
    unsigned a = __umulhi(r, owM);
    unsigned b = r - a * (unsigned)d.OW;
    if (b >= (unsigned)d.OW) { ++a; b -= (unsigned)d.OW; }
    const float* xn = d.x + (long)n * d.xsn;
    const float* dyp = dy + (long)n * dysn + (long)o0 * plane + r;
    const float* xc = xn + (int)a * d.Win + (int)b;
    float xv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = (int)a - 1 + ky, ix = (int)b - 1 + kx;
        xv[ky * 3 + kx] = ((unsigned)iy < (unsigned)d.Hin && (unsigned)ix < (unsigned)d.Win) ? xc[(ky - 1) * d.Win + (kx - 1)] : 0.f;
      }
#pragma unroll
    for (int oo = 0; oo < OG; ++oo) {
      const float g = dyp[(long)oo * plane];
      acc[oo][9] += g;
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[oo][k] = fmaf(g, xv[k], acc[oo][k]);
    }
  }
#pragma unroll
  for (int oo = 0; oo < OG; ++oo)
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      float v = acc[oo][k];
      for (int s2 = 32; s2 > 0; s2 >>= 1) v += __shfl_down(v, s2, 64);
      if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][oo * 10 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < OG * 10) {
    const int k = threadIdx.x;  // (channel oo = k / 10, sum k % 10)
    partial[((long)z * d.Cout + o0) * 10 + k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
  }
}

// one wavefront per (output channel, sum): lane z holds slice z, the shuffle tree adds them in a fixed order
static_assert(SCW_SLICES == 64, "smallcin_wgrad_fold_kernel: one lane per slice");
__global__ __launch_bounds__(640) void smallcin_wgrad_fold_kernel(const float* __restrict__ partial, int Cout, int K, float* gW,
                                                                  float* gb) {
  const int o = blockIdx.x, k = threadIdx.x >> 6, z = threadIdx.x & 63;
  float v = partial[((long)z * Cout + o) * 10 + k];
  for (int s2 = 32; s2 > 0; s2 >>= 1) v += __shfl_down(v, s2, 64);
  if (z != 0) return;
  if (k == 9) { if (gb) atomicAdd(gb + o, v); }
  else if (k < K) atomicAdd(gW + o * K + k, v);
}

size_t smallcin_wgrad_scratch_floats(int Cout) { return (size_t)SCW_SLICES * Cout * 10; }

void launch_smallcin_conv_wgrad(const SmallConvDesc& d, const float* dy, long dysn, float* gW, float* gb,
                                hipStream_t s, float* scratch, int* form_out) {
  if (dbm_abl_skip() & 128) return;  // (libdbm_measure.so only)
  const int K = d.Cin * d.KH * d.KW;
  // (the read-dy-once form serves conv_layer0's geometry only; everything else, and every call without scratch: one workgroup per element)
  if (scratch && (long)d.N * d.OH * d.OW >= 16384 && d.Cin == 1 && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.Cout % SCW_OG == 0) {
    hipLaunchKernelGGL(smallcin_wgrad_partial_kernel, dim3(d.Cout / SCW_OG, SCW_SLICES), dim3(256), 0, s, d, dy, dysn, scratch);
    hipLaunchKernelGGL(smallcin_wgrad_fold_kernel, dim3(d.Cout), dim3(640), 0, s, scratch, d.Cout, K, gW, gb);
    DBM_HIP(hipGetLastError());
    if (form_out) *form_out = 1;
    return;
  }
  if (form_out) *form_out = 0;
  hipLaunchKernelGGL(smallcin_conv_wgrad_kernel, dim3(d.Cout * K + (gb ? d.Cout : 0)), dim3(256), 0, s, d, dy, dysn, gW, gb);
  DBM_HIP(hipGetLastError());
}

// col[n][k][p] = x[n][c][a*s+ky][b*s+kx] for k = (c*KH+ky)*KW+kx < K, 0 for K <= k < KP (valid convolution, no padding).
// Turns the two wide-kernel input-block branches (k30 s10 on REMA, k6 s2 on MEaSUREs, srgan_train.py:231-246) into
// 900- / 72-deep GEMMs for the MFMA kernels; the OIHW weight flattening is exactly this k order.
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ x, float* __restrict__ col, int N, int Cin,
                                                     int Hin, int Win, int KH, int KW, int stride, int OH, int OW, int K,
                                                     int KP) {
  const int plane = OH * OW;
  const long total = (long)N * KP * plane;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int p = (int)(e % plane);
    const int k = (int)((e / plane) % KP);
    const int n = (int)(e / ((long)plane * KP));
    float v = 0.f;
    if (k < K) {
      const int c = k / (KH * KW), kr = k - c * KH * KW;
      const int ky = kr / KW, kx = kr - ky * KW;
      const int a = p / OW, b = p - a * OW;
      v = x[((long)n * Cin + c) * Hin * Win + (long)(a * stride + ky) * Win + b * stride + kx];
    }
    col[e] = v;
  }
}

void launch_im2col(const float* x, float* col, int N, int Cin, int Hin, int Win, int KH, int KW, int stride, int OH, int OW,
                   int KP, hipStream_t s) {
  if (dbm_abl_skip() & 256) return;  // (libdbm_measure.so only)
  const long total = (long)N * KP * OH * OW;
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(im2col_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, col, N, Cin, Hin, Win, KH, KW, stride, OH, OW,
                     Cin * KH * KW, KP);
  DBM_HIP(hipGetLastError());
}

// ----------------------------------------------------------------------------------------------
// backward of F.resize_images(mode="nearest") x2 (srgan_train.py:556-566): 2x2 sum pool, with the
// LeakyReLU derivative of the layer below fused in (mask = that layer's retained output, or null).
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumpool2_kernel(const float* __restrict__ g, const float* __restrict__ mask,
                                                       float* __restrict__ out, long total, int H, int W, float slope) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % W);
  const int y = (int)((e / W) % H);
  const long nc = e / ((long)W * H);
  const float* gp = g + (nc * 2 * H + 2 * y) * 2 * W + 2 * x;
  float v = (gp[0] + gp[1]) + (gp[2 * W] + gp[2 * W + 1]);
  if (mask) v = mask[e] >= 0.f ? v : slope * v;
  out[e] = v;
}

void launch_sumpool2(const float* g, const float* mask, float* out, long nc, int H, int W, float slope,
                     hipStream_t s) {
  const long total = nc * H * W;
  hipLaunchKernelGGL(sumpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, mask, out, total, H, W,
                     slope);
  DBM_HIP(hipGetLastError());
}


// chainer.dataset.concat_examples on a device-resident dataset: dst row i = src row idx[i] (rows of `row` elements of V)
template <typename V>
__global__ void gather_rows_kernel(const V* __restrict__ src, V* __restrict__ dst, const int* __restrict__ idx, long row) {
  const long i = blockIdx.y;
  const V* s = src + (long)idx[i] * row;
  V* d = dst + i * row;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < row; k += (long)gridDim.x * blockDim.x) d[k] = s[k];
}

void launch_gather_rows(const void* src, void* dst, const int* d_idx, int n, size_t row_bytes, hipStream_t s) {
  const bool wide = row_bytes % 16 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
  const long row = (long)(row_bytes / (wide ? 16 : 4));
  long gx = (row + 255) / 256;
  if (gx > 64) gx = 64;
  if (wide)
    hipLaunchKernelGGL(gather_rows_kernel<float4>, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, (const float4*)src, (float4*)dst,
                       d_idx, row);
  else
    hipLaunchKernelGGL(gather_rows_kernel<float>, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, s, (const float*)src, (float*)dst,
                       d_idx, row);
  DBM_HIP(hipGetLastError());
}
