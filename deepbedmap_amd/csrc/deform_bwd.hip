// Backward of the fused deformable layers (forwards: deform_fwd.hip, deform_window.hip): offset gradients, column gradients and the weight
// gradients of the 64 -> 64 and 64 -> 1 layers, from the same channels-last input and corner-table sampler (deform_tile.h).
#include "dbm_internal.h"
#include "kernels.h"
#include "deform_tile.h"
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Backward: offset gradients (+ the pieces that share their gathers).  The corner table additionally keeps the four
// one-dimensional weights, the corner validity and the coordinate-gradient masks.
//   deform_bwd64_fused_kernel  64 -> 64 layer: dcol = W^T dy per tap on the MFMAs (M = 64 in channels, N = 64 positions,
//                              K = 64 out channels) into an LDS tile, from there (a) to the column-gradient matrix the
//                              CSR gather kernel reads and (b) into the offset gradients -- replaces a 1x1 implicit
//                              GEMM writing 191 MB and deform_goff_kernel re-reading them
//   deform_bwd1_fused_kernel   64 -> 1 layer: dcol = w (x) gy is rank one; offset gradients and, from the same
//                              gathers, the layer's weight / bias gradient as per-workgroup partial sums
//                              (deform_wgrad1_fold_kernel adds them in workgroup order) -- the sample matrix of this
//                              layer is not needed at all
// ---------------------------------------------------------------------------------------------------------------
struct TileGeometryBwd {
  int4 idx[9 * DF_POS];     // pixel index n * plane + offset of the four corners (0 where outside the image)
  float4 wuv[9 * DF_POS];   // wu0, wu1, wv0, wv1
  int flags[9 * DF_POS];    // bits 0..3: corner inside the image, bit 4: mu, bit 5: mv
};

// (the tile walk and the deform_tap call are build_geometry's, deform_tile.h, word for word; only the fill of the entry differs.  Two
//  copies: sharing them -- the walk taking the fill as a lambda, or one function for an entry's sample -- changed the instructions of
//  every kernel that builds a table, 256-VGPR deform_bwd64_fused_kernel included)
__device__ __forceinline__ void build_geometry_bwd(TileGeometryBwd& g, const float* __restrict__ off, long offsn, long P0, long total,
                                                   int plane, int H, int W, int tid) {
  for (int e = tid; e < 9 * DF_POS; e += 256) {
    const int t = e >> 6, pl = e & 63;
    const long P = P0 + pl;
    int4 id = make_int4(0, 0, 0, 0);
    float4 wg = make_float4(0.f, 0.f, 0.f, 0.f);
    int fl = 0;
    if (P < total) {
      const int n = (int)(P / plane);
      const int p = (int)(P - (long)n * plane);
      const int a = p / W, b = p - a * W;
      const float* on = off + (long)n * offsn;
      const DeformTap s = deform_tap(on[(long)t * plane + p], on[(long)(9 + t) * plane + p], a, b, t / 3, t % 3, H, W);
      const int base = n * plane;
      if (s.o1 >= 0) { id.x = base + s.o1; fl |= 1; }
      if (s.o2 >= 0) { id.y = base + s.o2; fl |= 2; }
      if (s.o3 >= 0) { id.z = base + s.o3; fl |= 4; }
      if (s.o4 >= 0) { id.w = base + s.o4; fl |= 8; }
      if (s.g.mu) fl |= 16;
      if (s.g.mv) fl |= 32;
      wg = make_float4(s.g.wu0, s.g.wu1, s.g.wv0, s.g.wv1);
    }
    g.idx[e] = id;
    g.wuv[e] = wg;
    g.flags[e] = fl;
  }
}

__device__ __forceinline__ float4 mask4(const float4& v, bool ok) { return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f); }

// d sample / d u and d sample / d v of the four channels of a quad
__device__ __forceinline__ void coord_grads(const float4& wuv, const float4& x1, const float4& x2, const float4& x3, const float4& x4,
                                            float4& du, float4& dv) {
  const float wu0 = wuv.x, wu1 = wuv.y, wv0 = wuv.z, wv1 = wuv.w;
  du.x = deform_du(wv0, wv1, x1.x, x2.x, x3.x, x4.x);
  du.y = deform_du(wv0, wv1, x1.y, x2.y, x3.y, x4.y);
  du.z = deform_du(wv0, wv1, x1.z, x2.z, x3.z, x4.z);
  du.w = deform_du(wv0, wv1, x1.w, x2.w, x3.w, x4.w);
  dv.x = deform_dv(wu0, wu1, x1.x, x2.x, x3.x, x4.x);
  dv.y = deform_dv(wu0, wu1, x1.y, x2.y, x3.y, x4.y);
  dv.z = deform_dv(wu0, wu1, x1.z, x2.z, x3.z, x4.z);
  dv.w = deform_dv(wu0, wu1, x1.w, x2.w, x3.w, x4.w);
}

__device__ __forceinline__ float quad_sum16(float v) {  // over the sixteen channel quads of a position (lanes q = lane & 15)
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// gcol (N, 576, plane) = W^T gy (row c * 9 + t), goff (N, 18.., plane)[0:18] = offset gradients.  wb = the layer's
// per-tap transposed image [t][o][c] (IgLayer::wb[1] of the layer viewed as a 1x1 convolution): coalesced A operands.
__global__ __launch_bounds__(256, 2) void deform_bwd64_fused_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                 const float* __restrict__ wb, const float* __restrict__ gy,
                                                                 float* __restrict__ gcol, float* __restrict__ goff, int N, int H, int W,
                                                                 long offsn) {
  __shared__ TileGeometryBwd geo;
  __shared__ float dys[64 * DF_LD];  // [out channel][position]
  __shared__ float dcl[2][64 * DF_LD];  // [in channel][position] of the current tap, and of the previous one (its stores go out late)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const long P0 = (long)blockIdx.x * DF_POS;
  build_geometry_bwd(geo, off, offsn, P0, total, plane, H, W, tid);
  {  // the tile of gy: wavefront w stages out channels 16 w .., 256-byte runs along the positions
    const long P = P0 + lane;
    const bool pv = P < total;
    const long n = pv ? P / plane : 0;
    const float* src = gy + n * 64 * plane + (pv ? P - n * plane : 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) dys[(16 * wave + i) * DF_LD + lane] = pv ? src[(long)(16 * wave + i) * plane] : 0.f;
  }
  const int q = lane & 15, pi = lane >> 4;
  const float* xq = xt + 4 * q;
  const int ct = wave & 1, pt = wave >> 1, j = lane & 31, kh = lane >> 5;
  const float* wl = wb + (long)kh * 64 + ct * 32 + j;  // + (t * 64 + 2 op) * 64
  __syncthreads();
  // B operands (gy) do not depend on the tap; they are re-read from LDS in every tap (one ds_read_b32 per MFMA): 32 registers the
  // two-deep A operand needs
  const float* bsrc = dys + kh * DF_LD + pt * 32 + j;
  const long Ps = P0 + lane;
  const bool pvs = Ps < total;
  const long nsp = pvs ? Ps / plane : 0;
  // vmcnt counts loads AND stores, in order: a load issued behind a store can only be awaited by draining the store (a write round
  // trip, ~2 us) -- the first version of this loop did that nine times per workgroup (A operand of tap t + 1 behind the stores of tap t).
  // Now the column-gradient tile is double buffered in LDS and a tap's stores are issued inside the NEXT tap, behind that tap's
  // requests (corner gathers, the A operand of the tap AFTER it: two register sets) and in front of its MFMAs; every store is a
  // branch-free buffer store (offset -1 = dropped) so that hipcc keeps exact counts, and one barrier per tap is left.
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rgc = __builtin_amdgcn_make_buffer_rsrc(gcol, 0, (int)(4L * N * 576 * plane), 0x00020000);
  const __amdgpu_buffer_rsrc_t rgo = __builtin_amdgcn_make_buffer_rsrc(goff, 0, (int)(4L * ((long)(N - 1) * offsn + 18L * plane)), 0x00020000);
  // (buffer loads: 32-bit offsets, the tap / k part in an SGPR -- the 64-bit addresses of the flat forms cost this loop 40 registers)
  const __amdgpu_buffer_rsrc_t rwb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, 9 * 64 * 64 * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rxt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xt), 0, (int)(256L * total), 0x00020000);
  const int wl_off = 4 * (kh * 64 + ct * 32 + j);
  const int gcl0 = pvs ? (int)(4 * (nsp * 576 * plane + (Ps - nsp * plane))) : -1;
  const int pstride = 4 * plane;
  int go0[4];   // byte offset of (image, tap 0, position) of this thread's four offset-gradient positions; -1: not this lane's / outside
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long P = P0 + 16 * wave + 4 * i + pi;
    const long n = P < total ? P / plane : 0;
    go0[i] = (q == 0 && P < total) ? (int)(4 * (n * offsn + (P - n * plane))) : -1;
  }
  auto load_x = [&](int pix) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rxt, pix * 256 + 16 * q, 0, 0));
  };
  float gus[4], gvs[4];
  auto stores = [&](int t) {   // tap t's column gradients (256-byte runs along the positions) and offset gradients
    const float* src = dcl[t & 1] + lane;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = 16 * wave + i;
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, src[c * DF_LD]), rgc, gcl0 >= 0 ? gcl0 + (c * 9 + t) * pstride : -1, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gus[i]), rgo, go0[i] >= 0 ? go0[i] + t * pstride : -1, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gvs[i]), rgo, go0[i] >= 0 ? go0[i] + (9 + t) * pstride : -1, 0, 0);
    }
  };
  // A operand of tap t, k pairs [16 h, 16 h + 16)
  auto load_a = [&](float (&a)[16], int t, int h) {
#pragma unroll
    for (int op = 0; op < 16; ++op)
      a[op] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rwb, wl_off, 4 * (t * 64 + 2 * (16 * h + op)) * 64, 0));
  };
  // one tap: av = the first half of its A operand (requested a whole tap ago), avn = the next tap's first half, requested here with this
  // tap's second half (which has the first sixteen MFMAs to arrive) -- two full register sets do not fit beside the corner gathers
  auto tap = [&](int t, const float (&av)[16], float (&avn)[16]) {
    float4 c1[4], c2[4], c3[4], c4[4], cw[4];
    int fl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // the corner gathers of this tap: in flight underneath the MFMAs (CornerRequest's walk, as buffer loads)
      const int e = t * DF_POS + 16 * wave + 4 * i + pi;
      const int4 id = geo.idx[e];
      cw[i] = geo.wuv[e];
      fl[i] = geo.flags[e];
      c1[i] = load_x(id.x);
      c2[i] = load_x(id.y);
      c3[i] = load_x(id.z);
      c4[i] = load_x(id.w);
    }
    float avh[16];
    load_a(avh, t, 1);
    load_a(avn, t < 8 ? t + 1 : 8, 0);   // (the last tap re-reads its own: nothing uses it)
    __builtin_amdgcn_sched_barrier(0);
    if (t > 0) stores(t - 1);
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int op = 0; op < 16; ++op) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[op], bsrc[2 * op * DF_LD], acc, 0, 0, 0);
#pragma unroll
    for (int op = 0; op < 16; ++op) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(avh[op], bsrc[2 * (16 + op) * DF_LD], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    float* dc = dcl[t & 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) dc[DF_ACC_ROW(ct, kh, r) * DF_LD + pt * 32 + j] = acc[r];
    __syncthreads();
    // offset gradients
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pl = 16 * wave + 4 * i + pi;
      const float* dq = dc + (4 * q) * DF_LD + pl;
      const float4 g4 = make_float4(dq[0], dq[DF_LD], dq[2 * DF_LD], dq[3 * DF_LD]);
      float4 du, dv;
      coord_grads(cw[i], mask4(c1[i], fl[i] & 1), mask4(c2[i], fl[i] & 2), mask4(c3[i], fl[i] & 4), mask4(c4[i], fl[i] & 8), du, dv);
      const float gu = (g4.x * du.x + g4.y * du.y) + (g4.z * du.z + g4.w * du.w);
      const float gv = (g4.x * dv.x + g4.y * dv.y) + (g4.z * dv.z + g4.w * dv.w);
      const float su = quad_sum16(gu), sv = quad_sum16(gv);
      gus[i] = (fl[i] & 16) ? su : 0.f;
      gvs[i] = (fl[i] & 32) ? sv : 0.f;
    }
  };
  float a0[16], a1[16];
  load_a(a0, 0, 0);
#pragma unroll 1
  for (int t = 0; t < 8; t += 2) {
    tap(t, a0, a1);
    tap(t + 1, a1, a0);
  }
  tap(8, a0, a1);
  stores(8);
}

// goff as above with gcol = w[c*9+t] * gy[n][p]; partial (gridDim.x, 580): this workgroup's sums of gy * sample per
// (c * 9 + t), then of gy (the bias gradient) at [576].
__global__ __launch_bounds__(256) void deform_bwd1_fused_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                const float* __restrict__ w, const float* __restrict__ gy,
                                                                float* __restrict__ goff, float* __restrict__ partial, int N, int H, int W,
                                                                long offsn) {
  __shared__ TileGeometryBwd geo;
  __shared__ __attribute__((aligned(16))) float wsh[9 * 64];  // [tap][channel]
  __shared__ __attribute__((aligned(16))) float red[4][9 * 64];  // per wavefront: [tap][channel] sums of gy * sample
  __shared__ float gys[DF_POS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const long P0 = (long)blockIdx.x * DF_POS;
  build_geometry_bwd(geo, off, offsn, P0, total, plane, H, W, tid);
  for (int e = tid; e < 576; e += 256) wsh[(e % 9) * 64 + e / 9] = w[e];
  if (tid < DF_POS) gys[tid] = (P0 + tid < total) ? gy[P0 + tid] : 0.f;  // (N, 1, plane) is flat in the position index
  const int q = lane & 15, pi = lane >> 4;
  const float* xq = xt + 4 * q;
  __syncthreads();
  float gyv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) gyv[i] = gys[16 * wave + 4 * i + pi];
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    // (CornerRequest::request, deform_tile.h, on the backward table -- cw = wuv, + flags; its own copy: through the struct this kernel
    //  compiled to one instruction less and another schedule)
    float4 c1[4], c2[4], c3[4], c4[4], cw[4];
    int fl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t * DF_POS + 16 * wave + 4 * i + pi;
      const int4 id = geo.idx[e];
      cw[i] = geo.wuv[e];
      fl[i] = geo.flags[e];
      c1[i] = *reinterpret_cast<const float4*>(xq + (long)id.x * 64);
      c2[i] = *reinterpret_cast<const float4*>(xq + (long)id.y * 64);
      c3[i] = *reinterpret_cast<const float4*>(xq + (long)id.z * 64);
      c4[i] = *reinterpret_cast<const float4*>(xq + (long)id.w * 64);
    }
    const float4 wr = *reinterpret_cast<const float4*>(wsh + t * 64 + 4 * q);
    float4 ws = make_float4(0.f, 0.f, 0.f, 0.f);  // this lane's gy * sample of its four channels, over its four positions
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 x1 = mask4(c1[i], fl[i] & 1), x2 = mask4(c2[i], fl[i] & 2), x3 = mask4(c3[i], fl[i] & 4), x4 = mask4(c4[i], fl[i] & 8);
      float4 du, dv;
      coord_grads(cw[i], x1, x2, x3, x4, du, dv);
      const float g = gyv[i];
      float gu = g * ((wr.x * du.x + wr.y * du.y) + (wr.z * du.z + wr.w * du.w));
      float gv = g * ((wr.x * dv.x + wr.y * dv.y) + (wr.z * dv.z + wr.w * dv.w));
      gu = quad_sum16(gu);
      gv = quad_sum16(gv);
      const long P = P0 + 16 * wave + 4 * i + pi;
      if (q == 0 && P < total) {
        const long n = P / plane;
        float* gn = goff + n * offsn + (P - n * plane);
        gn[(long)t * plane] = (fl[i] & 16) ? gu : 0.f;
        gn[(long)(9 + t) * plane] = (fl[i] & 32) ? gv : 0.f;
      }
      const float4 sw = make_float4(cw[i].y * cw[i].w, cw[i].x * cw[i].w, cw[i].y * cw[i].z, cw[i].x * cw[i].z);  // w1..w4
      const float4 sm = blend4(sw, x1, x2, x3, x4);
      ws.x = fmaf(g, sm.x, ws.x); ws.y = fmaf(g, sm.y, ws.y); ws.z = fmaf(g, sm.z, ws.z); ws.w = fmaf(g, sm.w, ws.w);
    }
    // the four position groups of the wavefront (lanes q, q + 16, q + 32, q + 48)
    ws.x += __shfl_xor(ws.x, 16, 64); ws.y += __shfl_xor(ws.y, 16, 64); ws.z += __shfl_xor(ws.z, 16, 64); ws.w += __shfl_xor(ws.w, 16, 64);
    ws.x += __shfl_xor(ws.x, 32, 64); ws.y += __shfl_xor(ws.y, 32, 64); ws.z += __shfl_xor(ws.z, 32, 64); ws.w += __shfl_xor(ws.w, 32, 64);
    if (pi == 0) *reinterpret_cast<float4*>(&red[wave][t * 64 + 4 * q]) = ws;
  }
  __syncthreads();
  float* po = partial + (long)blockIdx.x * 580;
  for (int e = tid; e < 576; e += 256) {
    const int t = e >> 6, c = e & 63;
    po[c * 9 + t] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
  if (tid < 64) {
    float v = gys[tid];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (tid == 0) po[576] = v;
  }
}

// ---- weight gradient of the 64 -> 64 layer with the sampler fused in (round 6) ----
// gW[o][c][t] += sum_{n,p} gy[n][o][p] * sample(c, t, n, p);  gb[o] += sum gy.
// Until round 5 the retained forward wrote Chainer's sample matrix x_st (N, 576, plane): 191 MB at batch 64, written from the forward
// kernel's tap loop on the generator's critical path (deform64 "keep": 128 us against 112 without, 250 against 117 us INSIDE the
// iteration) and read back by a 1x1 weight-gradient GEMM on the side stream (102 us standalone, 212 MB).  This kernel re-samples instead:
// the forward kernel's sampler (corner table of the tile, sixteen lanes per 256-byte corner run, blend into a [channel][position] LDS
// tile, the next tap's gathers in flight under this tap's MFMAs) feeds MFMAs that contract over the tile's 64 POSITIONS: D[o][c] +=
// gy[o][p] * sample[c][p], one 32 x 32 accumulator tile per tap and wavefront (quadrant (o tile, c tile) = (wave & 1, wave >> 1)): nine
// tiles that live across the workgroup's tiles (persistent workgroups, strided tile assignment).  blockIdx.y = 0 / 1 takes taps 0..4 /
// 5..8: nine tiles (144 registers) beside the sampler's 80 spilled at two workgroups per CU; five fit.  Partial sums go to
// `partial` [workgroup][tap][o][c] (+ 64 bias sums), deform_wgrad64_fold_kernel adds them in workgroup order: deterministic.
__global__ __launch_bounds__(256, 2) void deform_wgrad64_fused_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                   const float* __restrict__ gy, float* __restrict__ partial, int N, int H,
                                                                   int W, long offsn, int ntiles) {
  __shared__ TileGeometry geo;
  __shared__ float col[2][64 * DF_LD];   // [buffer][channel][position]
  __shared__ float gys[64 * DF_LD];      // [out channel][position]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const long total = (long)N * plane;
  const int q = lane & 15, pi = lane >> 4;
  const float* xq = xt + 4 * q;
  const int ct = wave & 1, cq = wave >> 1, j = lane & 31, kh = lane >> 5;
  const int half = blockIdx.y;        // taps [5 half, 5 half + NT)
  f32x16 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;   // (half 0, threads 0..63: the bias gradient of out channel tid)
  // (its own copies of CornerRequest::request and ::write_samples, deform_tile.h: at 234 VGPRs under __launch_bounds__(256, 2) the struct
  //  schedules differently and takes 238)
  float4 c1[4], c2[4], c3[4], c4[4], cw[4];
  auto gather = [&](int t) {  // requests the four corners of this lane's channel quad at its four positions
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
  };
  auto blend = [&](float* dst) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = blend4(cw[i], c1[i], c2[i], c3[i], c4[i]);
      float* d = dst + (4 * q) * DF_LD + 16 * wave + 4 * i + pi;
      d[0] = v.x; d[DF_LD] = v.y; d[2 * DF_LD] = v.z; d[3 * DF_LD] = v.w;
    }
  };
  const float* asrc = gys + (ct * 32 + j) * DF_LD + kh;   // A[i = out channel][k = position parity]
#pragma unroll 1
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long P0 = (long)tile * DF_POS;
    __syncthreads();   // the previous tile's readers of geo / col / gys are done
    build_geometry(geo, off, offsn, P0, total, plane, H, W, tid, 0, 5 * half, half ? 9 : 5);   // (this half's taps only)
    {  // the tile of gy: wavefront w stages out channels 16 w .., 256-byte runs along the positions (positions past the end: zero)
      const long P = P0 + lane;
      const bool pv = P < total;
      const long n = pv ? P / plane : 0;
      const float* src = gy + n * 64 * plane + (pv ? P - n * plane : 0);
#pragma unroll
      for (int i = 0; i < 16; ++i) gys[(16 * wave + i) * DF_LD + lane] = pv ? src[(long)(16 * wave + i) * plane] : 0.f;
    }
    __syncthreads();
    gather(5 * half);
    blend(col[0]);
    __syncthreads();
    if (half == 0 && tid < 64) {   // bias gradient: this tile's 64 positions of out channel tid
      float a = 0.f;
#pragma unroll 8
      for (int pl = 0; pl < DF_POS; ++pl) a += gys[tid * DF_LD + pl];
      bsum += a;
    }
    // local tap u = 0..4 (u == 4 only in half 0): tap 5 half + u, LDS buffer u & 1
    auto multiply = [&](auto U_, bool more) {
      constexpr int u = decltype(U_)::value;
      if (more) gather(5 * half + u + 1);
      __builtin_amdgcn_sched_barrier(0);  // the requests above stay in front of the MFMA block they overlap
      const float* bsrc = col[u & 1] + (cq * 32 + j) * DF_LD + kh;   // B[k = position parity][j = in channel]
#pragma unroll
      for (int kk = 0; kk < 32; ++kk) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(asrc[2 * kk], bsrc[2 * kk], acc[u], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more) blend(col[(u + 1) & 1]);
      __syncthreads();
    };
    multiply(std::integral_constant<int, 0>{}, true);
    multiply(std::integral_constant<int, 1>{}, true);
    multiply(std::integral_constant<int, 2>{}, true);
    if (half == 0) {   // (uniform per workgroup)
      multiply(std::integral_constant<int, 3>{}, true);
      multiply(std::integral_constant<int, 4>{}, false);
    } else {
      multiply(std::integral_constant<int, 3>{}, false);
    }
  }
  // ---- this workgroup's partial sums: [tap][o][c], 128-byte runs along c (o = DF_ACC_ROW(ct, kh, r), written out: the macro's
  // parentheses associate the sum differently, and that costs this kernel an instruction) ----
  float* pw = partial + (size_t)blockIdx.x * (9 * 64 * 64 + 64);
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int t = 5 * half + u;
    if (t < 9) {
#pragma unroll
      for (int r = 0; r < 16; ++r) pw[(t * 64 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * 64 + cq * 32 + j] = acc[u][r];
    }
  }
  if (half == 0 && tid < 64) pw[9 * 64 * 64 + tid] = bsum;
}

// gw (64, 64, 3, 3) += sum over the workgroups' partial tiles, in workgroup order; gb (64) likewise
__global__ __launch_bounds__(256) void deform_wgrad64_fold_kernel(const float* __restrict__ partial, int nwg, float* gw, float* gb) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // index into a partial block: (t * 64 + o) * 64 + c, then 64 bias sums
  constexpr int PB = 9 * 64 * 64 + 64;
  if (e >= PB) return;
  float a = 0.f;
#pragma unroll 8
  for (int w = 0; w < nwg; ++w) a += partial[(size_t)w * PB + e];
  if (e < 9 * 64 * 64) {
    const int t = e / 4096, o = (e >> 6) & 63, c = e & 63;
    gw[(o * 64 + c) * 9 + t] += a;
  } else if (gb) {
    gb[e - 9 * 64 * 64] += a;
  }
}

// gw[k] += sum over workgroups of partial[wg][k], k < 576; gb[0] += ... [576].  One wavefront per output: lane l adds the
// workgroups l, l + 64, ... in order, the lanes fold with a fixed xor tree (reproducible).
__global__ __launch_bounds__(256) void deform_wgrad1_fold_kernel(const float* __restrict__ partial, int nwg, float* gw, float* gb) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k > 576) return;
  float a = 0.f;
  for (int g = lane; g < nwg; g += 64) a += partial[(long)g * 580 + k];
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) {
    if (k < 576) gw[k] += a;
    else if (gb) gb[0] += a;
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Round 5: the backward pass of the 64 -> 1 layer in the PREMULTIPLIED form the forward already uses (deform1_premul_kernel):
// with z_t = sum_c w[c][t] x_c (nine planes per image, kept from the forward pass) and G_t[q] = sum over the sampling
// entries (p, corner) that land on input pixel q of (bilinear weight x gy[p]) (nine planes, a CSR gather of ONE value),
//   d loss / d offset_t(p)  = gy[p] x (d bilinear z_t / d u, d v)          -- four single-float gathers per (p, t)
//   d loss / d x_c(q)       = sum_t w[c][t] G_t[q]
//   d loss / d w[c][t]      = sum_{n, q} x_c(q) G_t[q],   d loss / d b = sum gy
// -- no gather of 9 x 4 x 256 bytes per position any more (deform_bwd1_fused_kernel: 150 us at batch 64, the iteration's critical
// path) and the input-gradient gather moves 9 instead of 64 values per list entry.
// ---------------------------------------------------------------------------------------------------------------
// goff[n][t | 9 + t][p] from the forward's z planes: one thread per (position, tap)
__global__ __launch_bounds__(256) void deform1_goff_kernel(const float* __restrict__ z, const float* __restrict__ off,
                                                           const float* __restrict__ gy, float* __restrict__ goff, long total, int H, int W,
                                                           long offsn) {
  const long P = (long)blockIdx.x * 256 + threadIdx.x;
  if (P >= total) return;
  const int plane = H * W, t = blockIdx.y;
  const int n = (int)(P / plane);
  const int p = (int)(P - (long)n * plane);
  const int a = p / W, b = p - a * W;
  const float* on = off + (long)n * offsn + p;
  const DeformTap s = deform_tap(on[(long)t * plane], on[(long)(9 + t) * plane], a, b, t / 3, t % 3, H, W);
  const DeformGeom& g = s.g;
  const float* zt = z + ((long)n * 9 + t) * plane;
  const float z1 = s.o1 >= 0 ? zt[s.o1] : 0.f, z2 = s.o2 >= 0 ? zt[s.o2] : 0.f, z3 = s.o3 >= 0 ? zt[s.o3] : 0.f, z4 = s.o4 >= 0 ? zt[s.o4] : 0.f;
  float du, dv;   // (on the premultiplied corners)
  deform_coord_grads(g, z1, z2, z3, z4, du, dv);
  const float gv = gy[P];
  float* gn = goff + (long)n * offsn + p;
  gn[(long)t * plane] = g.mu ? gv * du : 0.f;
  gn[(long)(9 + t) * plane] = g.mv ? gv * dv : 0.f;
}

// gx[n][c][q] = sum_t w[c][t] G[n][t][q]; partial (gridDim.x, 580): this workgroup's sums of x_c(q) G_t(q) per (c * 9 + t), then of gy
// at [576] (folded by deform_wgrad1_fold_kernel in workgroup order).  Lane (q16, pi) owns four channels at four positions, as in the
// kernels above; xt is the layer input channels-last.
__global__ __launch_bounds__(256) void deform1_xw_kernel(const float* __restrict__ xt, const float* __restrict__ w, const float* __restrict__ G,
                                                         const float* __restrict__ gy, float* __restrict__ gx, float* __restrict__ partial,
                                                         long total, int plane) {
  __shared__ __attribute__((aligned(16))) float wsh[9 * 64];     // [tap][channel]
  __shared__ __attribute__((aligned(16))) float red[4][9 * 64];  // per wavefront: [tap][channel] sums of x * G
  __shared__ float gts[9][DF_POS];
  __shared__ float gys[DF_POS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long P0 = (long)blockIdx.x * DF_POS;
  for (int e = tid; e < 576; e += 256) wsh[(e % 9) * 64 + e / 9] = w[e];
  for (int e = tid; e < 9 * DF_POS; e += 256) {
    const int t = e / DF_POS, pl = e - t * DF_POS;
    const long P = P0 + pl;
    float v = 0.f;
    if (P < total) {
      const long n = P / plane;
      v = G[(n * 9 + t) * plane + (P - n * plane)];
    }
    gts[t][pl] = v;
  }
  if (tid < DF_POS) gys[tid] = (P0 + tid < total) ? gy[P0 + tid] : 0.f;
  __syncthreads();
  const int q = lane & 15, pi = lane >> 4;
  float4 xv[4];
  float4 gxv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long P = P0 + 16 * wave + 4 * i + pi;
    xv[i] = P < total ? *reinterpret_cast<const float4*>(xt + P * 64 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    gxv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const float4 wr = *reinterpret_cast<const float4*>(wsh + t * 64 + 4 * q);
    float4 ws = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float g = gts[t][16 * wave + 4 * i + pi];
      gxv[i].x = fmaf(wr.x, g, gxv[i].x); gxv[i].y = fmaf(wr.y, g, gxv[i].y); gxv[i].z = fmaf(wr.z, g, gxv[i].z); gxv[i].w = fmaf(wr.w, g, gxv[i].w);
      ws.x = fmaf(g, xv[i].x, ws.x); ws.y = fmaf(g, xv[i].y, ws.y); ws.z = fmaf(g, xv[i].z, ws.z); ws.w = fmaf(g, xv[i].w, ws.w);
    }
    ws.x += __shfl_xor(ws.x, 16, 64); ws.y += __shfl_xor(ws.y, 16, 64); ws.z += __shfl_xor(ws.z, 16, 64); ws.w += __shfl_xor(ws.w, 16, 64);
    ws.x += __shfl_xor(ws.x, 32, 64); ws.y += __shfl_xor(ws.y, 32, 64); ws.z += __shfl_xor(ws.z, 32, 64); ws.w += __shfl_xor(ws.w, 32, 64);
    if (pi == 0) *reinterpret_cast<float4*>(&red[wave][t * 64 + 4 * q]) = ws;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // gx is (N, 64, plane): a lane's four channels of one position
    const long P = P0 + 16 * wave + 4 * i + pi;
    if (P < total) {
      const long n = P / plane;
      float* dst = gx + (n * 64 + 4 * q) * plane + (P - n * plane);
      dst[0] = gxv[i].x; dst[plane] = gxv[i].y; dst[2L * plane] = gxv[i].z; dst[3L * plane] = gxv[i].w;
    }
  }
  __syncthreads();
  float* po = partial + (long)blockIdx.x * 580;
  for (int e = tid; e < 576; e += 256) {
    const int t = e >> 6, c = e & 63;
    po[c * 9 + t] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
  if (tid < 64) {
    float v = gys[tid];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (tid == 0) po[576] = v;
  }
}

}  // namespace

// Backward of the 64 -> 64 layer: gcol (N, 576, H, W) and goff[:, 0:18] are overwritten (the input gradient is then
// gathered from gcol by launch_deform_input_grad).  wb = IgLayer::wb[1] of the layer's 1x1 view ([tap][o][c]).
void launch_deform_bwd64_fused(const float* xt, const float* off, const float* wb, const float* gy, float* gcol, float* goff, int N, int H,
                               int W, long offsn, hipStream_t s) {
  const long total = (long)N * H * W;
  DBM_CHECK(total < (1L << 31), "fused deformable backward: more than 2^31 positions");
  DBM_CHECK(4L * total * 576 < (1L << 31) && 4L * N * offsn < (1L << 31), "fused deformable backward: column gradients beyond 2 GB (buffer accesses)");
  const unsigned blocks = (unsigned)((total + DF_POS - 1) / DF_POS);
  if (g_profiler.enabled) {
    char tag[40];
    snprintf(tag, sizeof(tag), "deform_bwd64_%dx%d_n%d", H, W, N);  // in: x, offsets, gy, weights; out: gcol (576 planes), goff
    g_profiler.begin(s, 0, 2.0 * (double)total * 64 * 576, 4.0 * ((double)total * (64 + 18 + 64 + 576 + 18) + 576.0 * 64), tag, blocks);
  }
  hipLaunchKernelGGL(deform_bwd64_fused_kernel, dim3(blocks), dim3(256), 0, s, xt, off, wb, gy, gcol, goff, N, H, W, offsn);
  if (g_profiler.enabled) g_profiler.end(s);
  DBM_HIP(hipGetLastError());
}

// Weight gradient of the 64 -> 64 deformable layer from the channels-last input, the offsets and gy (no sample matrix): gw (64, 64, 3, 3)
// and gb (64, may be null) are accumulated (+=) through `partial` (deform_wgrad64_partial_floats floats of scratch).
static int deform_wgrad64_wgs(long ntiles) {
  static const int n_cus = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    return prop.multiProcessorCount;
  }();
  return (int)(ntiles < n_cus ? ntiles : n_cus);   // x 2 tap halves = two resident workgroups per CU (68 KB of LDS each)
}
size_t deform_wgrad64_partial_floats(int N, int H, int W) {
  const long ntiles = ((long)N * H * W + DF_POS - 1) / DF_POS;
  return (size_t)deform_wgrad64_wgs(ntiles) * (9 * 64 * 64 + 64);
}
void launch_deform_wgrad64_fused(const float* xt, const float* off, const float* gy, float* gw, float* gb, float* partial, int N, int H, int W,
                                 long offsn, hipStream_t s) {
  const long total = (long)N * H * W;
  DBM_CHECK(total < (1L << 31), "fused deformable weight gradient: more than 2^31 positions");
  const long ntiles = (total + DF_POS - 1) / DF_POS;
  const int wgs = deform_wgrad64_wgs(ntiles);
  if (g_profiler.enabled) {
    char tag[40];
    snprintf(tag, sizeof(tag), "deform_wgrad64_%dx%d_n%d", H, W, N);  // in: x, offsets, gy; out: the partial tiles, the gradient
    g_profiler.begin(s, 1, 2.0 * (double)total * 64 * 576, 4.0 * ((double)total * (64 + 18 + 64) + 2.0 * wgs * (9 * 64 * 64 + 64) + 576.0 * 64), tag, wgs);
  }
  hipLaunchKernelGGL(deform_wgrad64_fused_kernel, dim3(wgs, 2), dim3(256), 0, s, xt, off, gy, partial, N, H, W, offsn, (int)ntiles);
  hipLaunchKernelGGL(deform_wgrad64_fold_kernel, dim3((9 * 64 * 64 + 64 + 255) / 256), dim3(256), 0, s, partial, wgs, gw, gb);
  if (g_profiler.enabled) g_profiler.end(s);
  DBM_HIP(hipGetLastError());
}

size_t deform_bwd1_partial_floats(int N, int H, int W) { return (size_t)(((long)N * H * W + DF_POS - 1) / DF_POS) * 580; }

// Backward of the 64 -> 1 layer: goff[:, 0:18] overwritten, gw (576, OIHW of (1, 64, 3, 3)) and gb accumulated (+=) through
// `partial` (deform_bwd1_partial_floats floats of scratch).
void launch_deform_bwd1_fused(const float* xt, const float* off, const float* w, const float* gy, float* goff, float* gw, float* gb,
                              float* partial, int N, int H, int W, long offsn, hipStream_t s) {
  const long total = (long)N * H * W;
  DBM_CHECK(total < (1L << 31), "fused deformable backward: more than 2^31 positions");
  const unsigned blocks = (unsigned)((total + DF_POS - 1) / DF_POS);
  hipLaunchKernelGGL(deform_bwd1_fused_kernel, dim3(blocks), dim3(256), 0, s, xt, off, w, gy, goff, partial, N, H, W, offsn);
  hipLaunchKernelGGL(deform_wgrad1_fold_kernel, dim3(145), dim3(256), 0, s, partial, (int)blocks, gw, gb);
  DBM_HIP(hipGetLastError());
}

// Backward of the 64 -> 1 deformable layer in the premultiplied form (round 5; see deform1_goff_kernel).  z: the forward's
// premultiplied planes (N, 9, plane); Gt: scratch of N * 9 * plane floats; csr_ws: deform_csr_workspace_floats floats;
// partial: deform_bwd1_partial_floats floats.  goff (N, >= 18, plane with image stride offsn) and gx (N, 64, plane) are overwritten,
// gw (576) / gb (1) accumulated.
void launch_deform_bwd1_premul(const float* xt, const float* off, const float* w, const float* gy, const float* z, float* goff, float* gx,
                               float* gw, float* gb, float* partial, float* csr_ws, float* Gt, int N, int H, int W, long offsn,
                               hipStream_t s, bool lists_built) {
  const long plane = (long)H * W, total = (long)N * plane;
  DBM_CHECK(total < (1L << 31), "deformable backward: more than 2^31 positions");
  const unsigned blocks = (unsigned)((total + DF_POS - 1) / DF_POS);
  hipLaunchKernelGGL(deform1_goff_kernel, dim3((unsigned)((total + 255) / 256), 9), dim3(256), 0, s, z, off, gy, goff, total, H, W, offsn);
  launch_deform_csr_gather1(off, gy, Gt, N, H, W, offsn, s, csr_ws, lists_built);
  hipLaunchKernelGGL(deform1_xw_kernel, dim3(blocks), dim3(256), 0, s, xt, w, Gt, gy, gx, partial, total, (int)plane);
  hipLaunchKernelGGL(deform_wgrad1_fold_kernel, dim3(145), dim3(256), 0, s, partial, (int)blocks, gw, gb);
  DBM_HIP(hipGetLastError());
}
