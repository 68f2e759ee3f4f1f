// The deformable 64 -> 64 forwards whose sampler reads an LDS WINDOW of the input instead of gathering from global memory: the fp32 form
// (deform_conv64_fusedw_kernel) and the split-bf16 form (deform_conv64_x3w_kernel), both software-pipelined by hand.  The gathering
// kernels they must agree with to the bit, and the launchers that choose between the two, are in deform_fwd.hip.
// This file alone is built with -mllvm -pragma-unroll-threshold=100000 (Makefile): both step loops must unroll completely.
#include "dbm_internal.h"
#include "kernels.h"
#include "deform_tile.h"
#include "deform_window.h"
#include <type_traits>

namespace {

constexpr int DW_PIX = 272;   // bytes between window pixels in LDS, both kernels: a pixel's 256 bytes + 16 of padding (see deform_conv64_x3w_kernel)

// The far lanes' half of a corner request, both kernels: the four corners' two 16-byte pieces from global memory (g1..g4: byte offsets
// of the corners from the image's first pixel xb; o0 / o1: the step's bytes inside a pixel) into the registers the LDS half names too.
#define DW_FAR_LOADS                                                                                                              \
  "global_load_dwordx4 %0, %[g1], %[xb] offset:%[o0]\n\tglobal_load_dwordx4 %1, %[g1], %[xb] offset:%[o1]\n\t"                     \
  "global_load_dwordx4 %2, %[g2], %[xb] offset:%[o0]\n\tglobal_load_dwordx4 %3, %[g2], %[xb] offset:%[o1]\n\t"                     \
  "global_load_dwordx4 %4, %[g3], %[xb] offset:%[o0]\n\tglobal_load_dwordx4 %5, %[g3], %[xb] offset:%[o1]\n\t"                     \
  "global_load_dwordx4 %6, %[g4], %[xb] offset:%[o0]\n\tglobal_load_dwordx4 %7, %[g4], %[xb] offset:%[o1]\n"

// ---- the 64 -> 64 layer's forward with the sampler on an LDS window, fp32 (round 6; the training tile's narrow planes) ----
// deform_conv64_fused_kernel (deform_fwd.hip) runs at 0.35 of the fp32 MFMA roof (111 us for 64 x 36 x 36 positions, 39 us of MFMAs): per tap it
// gathers 64 KB from global memory, blends them into an LDS tile behind a barrier and feeds the MFMAs one ds_read_b32 each.  Here (the
// idea of deform_conv64_x3w_kernel below, for planes narrow enough that a window of FULL rows fits) a workgroup of four wavefronts owns
// 128 consecutive positions of one image and stages every input row a sample with a vertical offset in [-2, 3) can touch -- <= 12 rows
// x (W + 7) pixels x 272 bytes (256 + padding: conflict-free corner reads) -- once; a wavefront owns 32 positions and BOTH
// output-channel tiles, lane (position j, k half kh) blends its position's channels of parity kh straight into the B operand: no sample
// tile, no barrier in the tap loop.  A sample whose rows leave the window (vertical offsets beyond the window; horizontally the window
// spans the whole padded row) reads global memory through the same generic pointer -- any offset is served.
// Blend expression, channel pairing per MFMA (2 cp, 2 cp + 1) and summation order (taps outer, channel pairs inner) are
// deform_conv64_fused_kernel's: the same bits.  No sample-matrix output (colout): the launcher keeps the older kernel for that.
// (DWF_R, DWF_POS, DWF_MAXPIX: deform_window.h -- the launcher's form choice reads them)
constexpr int DWF_LDS = DWF_MAXPIX * DW_PIX; // 143 616 bytes

__global__ __launch_bounds__(256) void deform_conv64_fusedw_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                   const float* __restrict__ wf, const float* __restrict__ bias,
                                                                   float* __restrict__ y, float* __restrict__ yt, int N, int H, int W,
                                                                   long offsn, int act, float slope, int tiles_per_image, int abl_arg) {
#ifdef DBM_MEASURE
  const int abl = abl_arg;   // (libdbm_measure.so, DBM_FUSEDW_ABL, results wrong: 1 no step loop, 2 no window staging, 8 no stores, 256 no MFMAs)
#else
  constexpr int abl = 0;
  (void)abl_arg;
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char fwin[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = H * W;
  const int n = blockIdx.x / tiles_per_image, tile = blockIdx.x - n * tiles_per_image;
  const int p0 = tile * DWF_POS, p1 = min(p0 + DWF_POS, plane) - 1;   // positions [p0, p1] of image n
  const int a0 = p0 / W, a1 = p1 / W;
  const int wy0 = a0 - 1 - DWF_R, NR = a1 - a0 + 1 + 2 * DWF_R + 3;   // window rows wy0 .. wy0 + NR - 1
  const int NC = W + 2 * DWF_R + 3, wx0 = -1 - DWF_R;                 // window columns: the whole padded row
  const int npix = NR * NC;
  const float* xn = xt + (long)n * plane * 64;
  // ---- the window: sixteen lanes per pixel (256 contiguous bytes), zeros outside the image.  ALL of a thread's pieces (<= 33) are
  // requested before the first is written: one workgroup per CU at one wavefront per SIMD has 512 registers per lane and nothing else to
  // hide a memory round trip behind (batches of eight: five round trips, 10 of a tile's 41 us) ----
  // (its own copy of the staging loop, as deform_conv64_x3w_kernel has: through one function both kernels compiled to other schedules)
  if (!(abl & 2)) {
    constexpr int NP = DWF_MAXPIX * 16 / 256;
    float4 st[NP];
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int u = it * 256 + tid, px = u >> 4, part = u & 15;
      const int hy = px / NC, hx = px - hy * NC;
      const int gy = wy0 + hy, gx = wx0 + hx;
      const bool inside = px < npix && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      st[it] = inside ? *reinterpret_cast<const float4*>(xn + ((long)gy * W + gx) * 64 + 4 * part) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int u = it * 256 + tid, px = u >> 4, part = u & 15;
      if (px < npix) *reinterpret_cast<float4*>(fwin + px * DW_PIX + part * 16) = st[it];
    }
  }
  // ---- this lane's position, its eighteen offsets, the nine taps' geometry (the block deform_conv64_x3w_kernel has too, each its own
  // copy: as one function -- and likewise open_tap below -- both kernels compiled to other schedules) ----
  const int j = lane & 31, kh = lane >> 5;
  const int p = p0 + 32 * wave + j;
  const bool valid = p <= p1;
  const int a = (valid ? p : p0) / W, b = (valid ? p : p0) - a * W;
  int pg[9];        // the top-left corner of tap t in image coordinates, packed (y0 + 2) << 16 | (x0 + 2)
  float4 cw[9];     // bilinear weights (build_geometry's: a corner outside the image has weight 0)
  {
    const float* on = off + (long)n * offsn + (valid ? p : p0);
    float ox[9], oy[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      ox[t] = on[(long)t * plane];
      oy[t] = on[(long)(9 + t) * plane];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const DeformGeom q = deform_geom(ox[t], oy[t], a, b, t / 3, t % 3, H, W, 1);
      const int y0 = q.v0 - 2, x0 = q.u0 - 2;   // image coordinates of the top-left corner (deform_corner: - pad - 1)
      const bool iy0 = (unsigned)y0 < (unsigned)H, iy1 = (unsigned)(y0 + 1) < (unsigned)H;
      const bool ix0 = (unsigned)x0 < (unsigned)W, ix1 = (unsigned)(x0 + 1) < (unsigned)W;
      cw[t].x = (valid && iy0 && ix0) ? q.wu1 * q.wv1 : 0.f;
      cw[t].y = (valid && iy0 && ix1) ? q.wu0 * q.wv1 : 0.f;
      cw[t].z = (valid && iy1 && ix0) ? q.wu1 * q.wv0 : 0.f;
      cw[t].w = (valid && iy1 && ix1) ? q.wu0 * q.wv0 : 0.f;
      pg[t] = ((y0 + 2) << 16) | (x0 + 2);
    }
  }
  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  __syncthreads();

  if (!(abl & 1)) {
    // ---- 72 pipelined steps (tap, eight channels): deform_conv64_x3w_kernel's loop (see there) with fp32 MFMAs.  Step s: wait for the
    // corner pieces of step s and the weights of step s - 1; request the corner pieces of step s + 1 (lanes inside the window: LDS, the
    // others: global memory under the complementary EXEC mask); blend the eight channels as four pairs in lock step, the eight MFMAs of
    // step s - 1 (four channel pairs (2 cp, 2 cp + 1) x two output-channel tiles) dealt between the stages; request the sixteen weights
    // of step s + 1.  A lane multiplies the channels of its parity: element kh of each blended pair.
    typedef float f4t __attribute__((ext_vector_type(4)));
    typedef float f2t __attribute__((ext_vector_type(2)));
    f4t C[2][8];
    float A[4][8];          // weights of a step: [channel pair i][output-channel tile ct] = A[.][2 i + ct]; requested TWO steps ahead (one
                            // wavefront per SIMD: nobody else hides an L2 round trip -- with one step the loop took 830 cycles per
                            // step even without its MFMAs), right behind the corner pieces: ONE wait count serves taps with and
                            // without far lanes (a branch between a request and its wait makes hipcc copy registers whose loads are
                            // still in flight: wrong results, measured)
    float pb[4];            // B operands of the step before (this lane's parity of its four channel pairs)
    const unsigned lbase = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)fwin;
    const unsigned wvo = (unsigned)(kh * 9 * 64 + j) * 4u;   // this lane's byte offset into wf: + (((2 cp) * 9 + t) * 64 + ct * 32) * 4
    unsigned t_lds = 0, t_g1 = 0, t_g2 = 0, t_g3 = 0, t_g4 = 0;
    unsigned long t_near = ~0ul;
    auto open_tap = [&](int t) {
      const int y0 = (pg[t] >> 16) - 2, x0 = (pg[t] & 0xffff) - 2;
      const int ry = y0 - wy0, rx = x0 - wx0;
      const bool near = (unsigned)ry < (unsigned)(NR - 1);   // (0 <= rx, rx + 1 < NC always: x0 in [-2, W])
      t_lds = lbase + (near ? (ry * NC + rx) * DW_PIX : 0);
      t_near = __builtin_amdgcn_ballot_w64(near);
      if (t_near != ~0ul) {   // (wave-uniform)
        const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1), xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
        t_g1 = (unsigned)(ya * W + xa) * 256u;
        t_g2 = (unsigned)(ya * W + xb) * 256u;
        t_g3 = (unsigned)(yb * W + xa) * 256u;
        t_g4 = (unsigned)(yb * W + xb) * 256u;
      }
    };
    // (the second / third / fourth corner's pixel lies NC - dependent bytes further: run-time distances, folded into the address registers)
    auto corners_ks = [&](auto KS, f4t (&c)[8]) {   // c[2 corner + e]
      constexpr int ks = decltype(KS)::value;   // channels 8 ks .. 8 ks + 7: bytes ks * 32 (+ 16)
      const unsigned ad1 = t_lds, ad2 = t_lds + DW_PIX, ad3 = t_lds + (unsigned)NC * DW_PIX, ad4 = ad3 + DW_PIX;
      const unsigned g1_ = t_g1, g2_ = t_g2, g3_ = t_g3, g4_ = t_g4;
      const unsigned long nm_ = t_near;
      const float* xb_ = xn;
      // ONE asm statement for both kinds of lanes (the far lanes' loads skipped by a branch INSIDE it when there are none): two
      // statements in the arms of an if would define the same registers twice, and hipcc may then copy them at the join -- before the
      // wait, while the loads are still in flight
      unsigned long sv;
      asm volatile("s_mov_b64 %[sv], exec\n\ts_and_b64 exec, %[sv], %[nm]\n\ts_cbranch_execz .Lfw_nolds%=\n\t"
                   "ds_read_b128 %0, %[a1] offset:%[o0]\n\tds_read_b128 %1, %[a1] offset:%[o1]\n\t"
                   "ds_read_b128 %2, %[a2] offset:%[o0]\n\tds_read_b128 %3, %[a2] offset:%[o1]\n\t"
                   "ds_read_b128 %4, %[a3] offset:%[o0]\n\tds_read_b128 %5, %[a3] offset:%[o1]\n\t"
                   "ds_read_b128 %6, %[a4] offset:%[o0]\n\tds_read_b128 %7, %[a4] offset:%[o1]\n"
                   ".Lfw_nolds%=:\n\t"
                   "s_andn2_b64 exec, %[sv], %[nm]\n\ts_cbranch_execz .Lfw_nofar%=\n\t"
                   DW_FAR_LOADS
                   ".Lfw_nofar%=:\n\t"
                   "s_mov_b64 exec, %[sv]"
                   : "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3]), "=&v"(c[4]), "=&v"(c[5]), "=&v"(c[6]), "=&v"(c[7]), [sv] "=&s"(sv)
                   : [a1] "v"(ad1), [a2] "v"(ad2), [a3] "v"(ad3), [a4] "v"(ad4), [nm] "s"(nm_), [g1] "v"(g1_), [g2] "v"(g2_), [g3] "v"(g3_),
                     [g4] "v"(g4_), [xb] "s"(xb_), [o0] "n"(ks * 32), [o1] "n"(ks * 32 + 16)
                   : "scc");
    };
    auto request_corners = [&](int st, f4t (&c)[8]) {
      if ((st & 7) == 0) open_tap(st >> 3);
      switch (st & 7) {
        case 0: corners_ks(std::integral_constant<int, 0>{}, c); break;
        case 1: corners_ks(std::integral_constant<int, 1>{}, c); break;
        case 2: corners_ks(std::integral_constant<int, 2>{}, c); break;
        case 3: corners_ks(std::integral_constant<int, 3>{}, c); break;
        case 4: corners_ks(std::integral_constant<int, 4>{}, c); break;
        case 5: corners_ks(std::integral_constant<int, 5>{}, c); break;
        case 6: corners_ks(std::integral_constant<int, 6>{}, c); break;
        default: corners_ks(std::integral_constant<int, 7>{}, c); break;
      }
    };
    // the sixteen weights of step st = (tap t, channels 8 ks ..): channel pairs cp = 4 ks + i, rows ((2 cp) * 9 + t) of wf (+ kh * 9: wvo)
    auto request_weights = [&](int st, float (&aw)[8]) {
      const int t = st >> 3, ks = st & 7;
      const float* b0 = wf + ((long)(2 * (4 * ks + 0)) * 9 + t) * 64;
      const float* b1 = wf + ((long)(2 * (4 * ks + 1)) * 9 + t) * 64;
      const float* b2 = wf + ((long)(2 * (4 * ks + 2)) * 9 + t) * 64;
      const float* b3 = wf + ((long)(2 * (4 * ks + 3)) * 9 + t) * 64;
      const unsigned vo = wvo;
      asm volatile("global_load_dword %0, %[vo], %[b0]\n\tglobal_load_dword %1, %[vo], %[b0] offset:128\n\t"
                   "global_load_dword %2, %[vo], %[b1]\n\tglobal_load_dword %3, %[vo], %[b1] offset:128\n\t"
                   "global_load_dword %4, %[vo], %[b2]\n\tglobal_load_dword %5, %[vo], %[b2] offset:128\n\t"
                   "global_load_dword %6, %[vo], %[b3]\n\tglobal_load_dword %7, %[vo], %[b3] offset:128"
                   : "=&v"(aw[0]), "=&v"(aw[1]), "=&v"(aw[2]), "=&v"(aw[3]), "=&v"(aw[4]), "=&v"(aw[5]), "=&v"(aw[6]), "=&v"(aw[7])
                   : [vo] "v"(vo), [b0] "s"(b0), [b1] "s"(b1), [b2] "s"(b2), [b3] "s"(b3));
    };
#define DWF_THROUGH(c, aw) "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(aw[0]), "+v"(aw[1]), \
                           "+v"(aw[2]), "+v"(aw[3]), "+v"(aw[4]), "+v"(aw[5]), "+v"(aw[6]), "+v"(aw[7])
    // MFMA k (0..7) of the step whose weights are aw: channel pair i = k >> 1, output-channel tile ct = k & 1
    auto mfma_k = [&](int k, const float (&aw)[8]) {
      if (abl & 256) return;
      acc[k & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[k], pb[k >> 1], acc[k & 1], 0, 0, 0);
    };
    constexpr int NST = 72;
    request_corners(0, C[0]);
    request_weights(0, A[0]);
    request_weights(1, A[1]);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      f4t (&c)[8] = C[st & 1];
      float (&aw)[8] = A[(st + 3) & 3];    // the weights of step st - 1
      // Needed now: the corner pieces of step st (LDS: lgkmcnt(0); the global pieces of its far lanes, if the tap has any) and the weights
      // of step st - 1.  In issue order: ... corner pieces(st) [step st - 1], weights(st + 1) [step st - 1, right behind them]: the
      // youngest eight loads stay in flight (step 0: both weight requests of the prologue; the last step: nothing is younger).
      if (st == 0) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" : DWF_THROUGH(c, aw));
      else if (st + 1 < NST) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" : DWF_THROUGH(c, aw));
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : DWF_THROUGH(c, aw));
      if (st + 1 < NST) request_corners(st + 1, C[(st + 1) & 1]);
      if (st + 2 < NST) request_weights(st + 2, A[(st + 2) & 3]);
      auto mfma = [&](int k) {
        if (st > 0) mfma_k(k, aw);
      };
      const float4 w = cw[st >> 3];
      f2t m[4];
#define DWF_FENCE asm volatile("" : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]))
#define DWF_PAIR(q, k) ((f2t){c[q + (k >> 1)][2 * (k & 1)], c[q + (k >> 1)][2 * (k & 1) + 1]})   /* corner q / 2, channel pair k of the eight */
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = w.y * DWF_PAIR(2, k);
      DWF_FENCE;
      mfma(0); mfma(1);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = __builtin_elementwise_fma((f2t){w.x, w.x}, DWF_PAIR(0, k), m[k]);
      DWF_FENCE;
      mfma(2); mfma(3);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = __builtin_elementwise_fma((f2t){w.z, w.z}, DWF_PAIR(4, k), m[k]);
      DWF_FENCE;
      mfma(4); mfma(5);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = __builtin_elementwise_fma((f2t){w.w, w.w}, DWF_PAIR(6, k), m[k]);
      DWF_FENCE;
      mfma(6); mfma(7);
#undef DWF_FENCE
#undef DWF_PAIR
#pragma unroll
      for (int k = 0; k < 4; ++k) pb[k] = kh ? m[k][1] : m[k][0];
    }
    {  // the last step's MFMAs
      float (&aw)[8] = A[(NST - 1) & 3];
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(aw[0]), "+v"(aw[1]), "+v"(aw[2]), "+v"(aw[3]), "+v"(aw[4]), "+v"(aw[5]), "+v"(aw[6]), "+v"(aw[7]));
#pragma unroll
      for (int k = 0; k < 8; ++k) mfma_k(k, aw);
    }
#undef DWF_THROUGH
  }
  if (!valid || (abl & 8)) return;
  const long Pm = (long)n * plane + p;
  float v[2][16];   // (all bias loads before the first store: see DF_EPILOGUE64_VALUES)
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) DF_EPILOGUE64_VALUES(v[ct], acc[ct], ct, kh, bias, act, slope)
  if (y) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) DF_EPILOGUE64_STORE_Y(v[ct], ct, kh, y, (long)n * 64 * plane + p, plane)
  }
  if (yt) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) DF_EPILOGUE64_STORE_YT(v[ct], ct, kh, yt + Pm * 64)
  }
}

// ---- the same layer with the sampler reading an LDS WINDOW of the input (round 6; the bf16 sweep's full-resolution planes) ----
// deform_conv64_x3_kernel gathers four corners x 256 bytes per position and tap from the vector L1: 12 GB per 1144 x 1144 plane, 0.8 of the
// 4.8 ms of a crop.  Neighbouring positions and taps share almost all of those corners as long as the offsets are a few pixels: here a
// workgroup owns a 16 x 16 tile of positions and stages the input pixels every sample with offsets in [-2, 3) can touch -- the tile, one
// ring for the 3 x 3 taps, DW_R rings for the offsets, one more row / column for the bilinear neighbour: 23 x 23 pixels x 256 bytes (fp32,
// all 64 channels) = 132 KB, once -- 2.07 pixels staged per position instead of 36 gathered.
//   * LDS layout: pixel p (row-major in the window) at p * 272: its 256 bytes + 16 of padding.  The lanes of a ds_read_b128 group hold
//     sixteen consecutive positions of a row, whose corners are (for smooth offsets) consecutive pixels: 272 bytes apart = four banks
//     further each, sixteen of them = all 64 banks.  Padding, not an XOR swizzle: a lane's 32 reads per tap (four corners x eight
//     16-byte parts) are then ONE base register + immediate offsets -- the first version spent two VALU instructions per read on swizzled
//     addresses (2 700 VALU instructions per lane and tile, more cycles than its MFMAs, LDS reads or weight loads);
//     staged through registers (LDS-DMA writes a wavefront's 1 KB contiguously: no padding).
//   * no sample tile, no geometry table, no barrier inside the tap loop: a wavefront owns two rows of the tile (32 positions, dealt to
//     the lanes by the ds_read_b128 groups as in conv_cl16.hip) and BOTH output-channel tiles; lane (j, kg) samples the eight channels
//     16 ks + 8 kg .. + 7 of its position straight into the B operand of the k step (blend in fp32, split hi / lo in registers).
//   * 36 steps (tap, k step), software-pipelined by hand (see the loop): corner pieces and weight fragments requested a step ahead, the
//     blend as four channel pairs in lock step, the previous step's MFMAs dealt between its stages.
//   * arithmetic and summation order are deform_conv64_x3_kernel's (same blend expression, same split, taps outer, k steps inner, the
//     three products small terms first): the results are the same bits.
//   * a sample that leaves the window (offsets beyond DW_R) is served INSIDE the same loop: per tap the lanes whose four corners lie in
//     the window read LDS, the others read the same bytes from global memory under the complementary EXEC mask, one step ahead like
//     everything else -- any offset is served, the window is an accelerator.  (A first version sent the whole wavefront to an
//     unpipelined loop as soon as one of its 288 samples left the window: with offsets of about a pixel -- tools/dem_model.py --
//     that is every wavefront, and the continent sweep was SLOWER than with the gathering kernel: 1.86 against 1.76 s; now 1.60.)
// (DW_T, the tile edge: deform_window.h)
constexpr int DW_R = 2;                           // offsets in [-DW_R, DW_R + 1) stay inside the window
constexpr int DW_WIN = DW_T + 2 * DW_R + 3;       // 23
constexpr int DW_NPIX = DW_WIN * DW_WIN;          // 529
constexpr int DW_LDS = DW_NPIX * DW_PIX;          // 143 888 bytes
constexpr int DW_STEPS = (DW_NPIX * 16 + 511) / 512;   // 16-byte pieces per thread

// half-lane h (0..31) -> (row 0/1, column 0..15) of the wavefront's 2 x 16 patch: each 16-lane group of a ds_read_b128
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}: MI355X_MICROARCH.md, LDS) covers one row (conv_cl16.hip's patch_of)
__device__ __forceinline__ void dw_patch_of(int h, int& g, int& i) {
  if (h < 4) { g = 0; i = h; }
  else if (h < 12) { g = 1; i = h - 4; }
  else if (h < 16) { g = 0; i = h - 8; }
  else if (h < 20) { g = 1; i = h - 8; }
  else if (h < 28) { g = 0; i = h - 12; }
  else { g = 1; i = h - 16; }
}

__global__ __launch_bounds__(512) void deform_conv64_x3w_kernel(const float* __restrict__ xt, const float* __restrict__ off,
                                                                const dbf16x8* __restrict__ wx, const float* __restrict__ bias,
                                                                float* __restrict__ y, float* __restrict__ yt, int N, int H, int W,
                                                                long offsn, int act, float slope, int tilesX, int tilesY, int abl_arg) {
#ifdef DBM_MEASURE
  const int abl = abl_arg;   // (a run-time value costs a dozen branches per step: libdbm_measure.so's times are ~5 % above the product's)
#else
  constexpr int abl = 0;
  (void)abl_arg;
#endif
  // (abl: libdbm_measure.so only, DBM_X3W_ABL, results wrong: 1 no step loop, 2 no window staging, 4 no geometry, 8 no stores,
  //  16 every step's weight fragments are step 0's, 32 no weight loads, 64 no corner reads, 128 no blend arithmetic, 256 no MFMAs)
  extern __shared__ __attribute__((aligned(16))) unsigned char win[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // workgroup -> tile: every XCD (workgroups are dealt to the eight XCDs round robin) takes one contiguous run of tiles -- neighbouring
  // tiles share window rows and columns in that XCD's L2
  unsigned b = blockIdx.x;
  {
    const unsigned per = gridDim.x >> 3, rem = gridDim.x & 7, x = b & 7, k = b >> 3;
    b = x * per + (x < rem ? x : rem) + k;
  }
  const int tx = (int)(b % (unsigned)tilesX);
  b /= (unsigned)tilesX;
  const int ty = (int)(b % (unsigned)tilesY), n = (int)(b / (unsigned)tilesY);
  const int plane = H * W;
  const int wy0 = ty * DW_T - 1 - DW_R, wx0 = tx * DW_T - 1 - DW_R;   // image coordinates of window pixel (0, 0)
  const float* xn = xt + (long)n * plane * 64;
  // (the staging loop of deform_conv64_fusedw_kernel with this kernel's constants; one function for both changed both schedules)
  if (!(abl & 2)) {  // ---- the window: sixteen lanes per pixel (256 contiguous bytes), zeros outside the image ----
    float4 st[DW_STEPS];
#pragma unroll
    for (int it = 0; it < DW_STEPS; ++it) {
      const int u = it * 512 + tid, px = u >> 4, part = u & 15;
      const int hy = px / DW_WIN, hx = px - hy * DW_WIN;
      const int gy = wy0 + hy, gx = wx0 + hx;
      const bool inside = px < DW_NPIX && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      st[it] = inside ? *reinterpret_cast<const float4*>(xn + ((long)gy * W + gx) * 64 + 4 * part) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < DW_STEPS; ++it) {
      const int u = it * 512 + tid, px = u >> 4, part = u & 15;
      if (px < DW_NPIX) *reinterpret_cast<float4*>(win + px * DW_PIX + part * 16) = st[it];
    }
  }
  // ---- this lane's position, its eighteen offsets, the nine taps' geometry (deform_conv64_fusedw_kernel's block and its open_tap,
  // copied: see there) ----
  int g, i;
  dw_patch_of(lane & 31, g, i);
  const int kg = lane >> 5;
  const int a = ty * DW_T + 2 * wave + g, bcol = tx * DW_T + i;
  const bool valid = a < H && bcol < W;
  const int p = a * W + bcol;
  int pg[9];        // the top-left corner of tap t in image coordinates, packed (y0 + 2) << 16 | (x0 + 2)  (y0, x0 >= -2)
  float4 cw[9];     // bilinear weights (build_geometry's: a corner outside the image has weight 0)
  if (abl & 4) {
#pragma unroll
    for (int t = 0; t < 9; ++t) { pg[t] = ((wy0 + 2 + 2) << 16) | (wx0 + 2 + 2); cw[t] = make_float4(0.f, 0.f, 0.f, 0.f); }
  } else {
    const float* on = off + (long)n * offsn + (valid ? p : 0);
    float ox[9], oy[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      ox[t] = on[(long)t * plane];
      oy[t] = on[(long)(9 + t) * plane];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const DeformGeom q = deform_geom(ox[t], oy[t], a, bcol, t / 3, t % 3, H, W, 1);
      const int y0 = q.v0 - 2, x0 = q.u0 - 2;   // image coordinates of the top-left corner (deform_corner: - pad - 1)
      const bool iy0 = (unsigned)y0 < (unsigned)H, iy1 = (unsigned)(y0 + 1) < (unsigned)H;
      const bool ix0 = (unsigned)x0 < (unsigned)W, ix1 = (unsigned)(x0 + 1) < (unsigned)W;
      cw[t].x = (valid && iy0 && ix0) ? q.wu1 * q.wv1 : 0.f;
      cw[t].y = (valid && iy0 && ix1) ? q.wu0 * q.wv1 : 0.f;
      cw[t].z = (valid && iy1 && ix0) ? q.wu1 * q.wv0 : 0.f;
      cw[t].w = (valid && iy1 && ix1) ? q.wu0 * q.wv0 : 0.f;
      pg[t] = ((y0 + 2) << 16) | (x0 + 2);
    }
  }
  const dbf16x8* wl = wx + lane;   // + ((t * 4 + ks) * 2 + hl) * 128 + ct * 64
  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  __syncthreads();

  if (!(abl & 1)) {
    // ---- 36 pipelined steps (tap, k step) ----
    // The reads are inline asm with hand-placed wait counts: left to hipcc every read ends up right in front of its first use (its IR
    // passes sink loads through __builtin_amdgcn_sched_barrier; volatile loads turn into flat loads with a wait each); the values pass
    // through the wait as "+v" operands, so that nothing using them can move above it.  Step s:
    //   wait: the corner pieces of step s and the weight fragments of step s - 1 (vmcnt / lgkmcnt count in order: everything but the
    //     four fragment loads of step s, the youngest requests);
    //   the corner pieces of step s + 1 requested (their own double buffer): lanes whose four corners lie inside the window read LDS,
    //     the others -- offsets beyond DW_R -- read the same bytes from global memory, in the same instruction slot under the
    //     complementary EXEC mask (wave-uniform: a tap without such lanes issues the LDS reads only).  Any offset is served, at the
    //     speed of its locality;
    //   blend + split of step s as four channel PAIRS in lock step, the six MFMAs of step s - 1 dealt between its stages -- a wavefront's
    //     matrix instructions run under its own vector arithmetic (left to hipcc: one pair after the other through the same two
    //     registers, eight dependent packed operations deep with a wait state between each, then six MFMAs back to back).  The empty
    //     asm statements are ordering fences: every pair's operation k before any pair's operation k + 1, MFMA k between stage k and
    //     stage k + 1 (its B operands pass through both fences);
    //   the weight fragments of step s + 1 requested into the registers the MFMAs just read.
    // Same expression trees as blend4 / the gathering kernel's split, same MFMA order per accumulator: the same bits.
    typedef float f4t __attribute__((ext_vector_type(4)));
    typedef float f2t __attribute__((ext_vector_type(2)));
    f4t C[2][8], A[2][4];
    dbf16x8 pbh, pbl;   // B operands of the step before
    const unsigned lbase = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)win;
    const unsigned char* wp = reinterpret_cast<const unsigned char*>(wl);   // + 4096 per step; hi ct 0 / hi ct 1 / lo ct 0 / lo ct 1: + 0 / 1024 / 2048 / 3072
    // the tap whose corners are being requested: LDS address (lanes inside the window), byte offsets of the four corners from the
    // image's first pixel (the others; a corner outside the image is clamped onto it: its weight is 0), the lanes inside
    unsigned t_lds = 0, t_g1 = 0, t_g2 = 0, t_g3 = 0, t_g4 = 0;
    unsigned long t_near = ~0ul;
    auto open_tap = [&](int t) {
      const int y0 = (pg[t] >> 16) - 2, x0 = (pg[t] & 0xffff) - 2;
      const int ry = y0 - wy0, rx = x0 - wx0;
      const bool near = (unsigned)ry < (unsigned)(DW_WIN - 1) && (unsigned)rx < (unsigned)(DW_WIN - 1);
      t_lds = lbase + (near ? (ry * DW_WIN + rx) * DW_PIX : 0) + kg * 32;
      t_near = __builtin_amdgcn_ballot_w64(near);
      if (t_near != ~0ul) {   // (wave-uniform)
        const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1), xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
        t_g1 = (unsigned)(ya * W + xa) * 256u + kg * 32;
        t_g2 = (unsigned)(ya * W + xb) * 256u + kg * 32;
        t_g3 = (unsigned)(yb * W + xa) * 256u + kg * 32;
        t_g4 = (unsigned)(yb * W + xb) * 256u + kg * 32;
      }
    };
#define DW_LDS_READS "ds_read_b128 %0, %[ad] offset:%[k0]\n\tds_read_b128 %1, %[ad] offset:%[k1]\n\t" \
                     "ds_read_b128 %2, %[ad] offset:%[k2]\n\tds_read_b128 %3, %[ad] offset:%[k3]\n\t" \
                     "ds_read_b128 %4, %[ad] offset:%[k4]\n\tds_read_b128 %5, %[ad] offset:%[k5]\n\t" \
                     "ds_read_b128 %6, %[ad] offset:%[k6]\n\tds_read_b128 %7, %[ad] offset:%[k7]"
#define DW_LDS_OFFS(KS) [k0] "n"(KS * 64), [k1] "n"(KS * 64 + 16), [k2] "n"(KS * 64 + DW_PIX), [k3] "n"(KS * 64 + DW_PIX + 16), \
                        [k4] "n"(KS * 64 + DW_WIN * DW_PIX), [k5] "n"(KS * 64 + DW_WIN * DW_PIX + 16), \
                        [k6] "n"(KS * 64 + (DW_WIN + 1) * DW_PIX), [k7] "n"(KS * 64 + (DW_WIN + 1) * DW_PIX + 16)
    auto corners_ks = [&](auto KS, f4t (&c)[8]) {   // c[2 corner + e]
      constexpr int ks = decltype(KS)::value;
      if (abl & 64) return;   // (64: no corner reads)
      // (copies: clang does not capture a variable a generic lambda names in asm operands only)
      const unsigned ad_ = t_lds, g1_ = t_g1, g2_ = t_g2, g3_ = t_g3, g4_ = t_g4;
      const unsigned long nm_ = t_near;
      const float* xb_ = xn;
      // ONE asm statement for both kinds of lanes (the far lanes' loads skipped by a branch INSIDE it when there are none): two
      // statements in the arms of an if would define the same registers twice, and hipcc may then copy them at the join -- before the
      // wait, while the loads are still in flight (it did, in deform_conv64_fusedw_kernel's first two-armed wait)
      unsigned long sv;
      asm volatile("s_mov_b64 %[sv], exec\n\ts_and_b64 exec, %[sv], %[nm]\n\ts_cbranch_execz .Lxw_nolds%=\n\t" DW_LDS_READS "\n"
                   ".Lxw_nolds%=:\n\t"
                   "s_andn2_b64 exec, %[sv], %[nm]\n\ts_cbranch_execz .Lxw_nofar%=\n\t"
                   DW_FAR_LOADS
                   ".Lxw_nofar%=:\n\t"
                   "s_mov_b64 exec, %[sv]"
                   : "=&v"(c[0]), "=&v"(c[1]), "=&v"(c[2]), "=&v"(c[3]), "=&v"(c[4]), "=&v"(c[5]), "=&v"(c[6]), "=&v"(c[7]), [sv] "=&s"(sv)
                   : [ad] "v"(ad_), DW_LDS_OFFS(ks), [nm] "s"(nm_), [g1] "v"(g1_), [g2] "v"(g2_), [g3] "v"(g3_), [g4] "v"(g4_),
                     [xb] "s"(xb_), [o0] "n"(ks * 64), [o1] "n"(ks * 64 + 16)
                   : "scc");
    };
    auto request_corners = [&](int st, f4t (&c)[8]) {
      if ((st & 3) == 0) open_tap(st >> 2);
      switch (st & 3) {
        case 0: corners_ks(std::integral_constant<int, 0>{}, c); break;
        case 1: corners_ks(std::integral_constant<int, 1>{}, c); break;
        case 2: corners_ks(std::integral_constant<int, 2>{}, c); break;
        default: corners_ks(std::integral_constant<int, 3>{}, c); break;
      }
    };
    auto request_weights = [&](int st, f4t (&aw)[4]) {
      const unsigned char* q = wp + (long)((abl & 16) ? 0 : st) * 4096;   // (16: every step multiplies by step 0's fragments)
      if (abl & 32) return;                                                  // (32: no weight loads at all)
      asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:1024\n\t"
                   "global_load_dwordx4 %2, %4, off offset:2048\n\tglobal_load_dwordx4 %3, %4, off offset:3072"
                   : "=&v"(aw[0]), "=&v"(aw[1]), "=&v"(aw[2]), "=&v"(aw[3])
                   : "v"(q));
    };
#define DW_THROUGH(c, aw) "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(aw[0]), "+v"(aw[1]), \
                          "+v"(aw[2]), "+v"(aw[3])
    // MFMA k of the step whose fragments are aw (per accumulator: hi * lo, lo * hi, hi * hi -- small terms first)
    auto mfma_k = [&](int k, const f4t (&aw)[4]) {
      const int ct = k & 1;
      const dbf16x8 av = __builtin_bit_cast(dbf16x8, aw[k < 2 ? ct : k < 4 ? 2 + ct : ct]);   // hi ct 0, hi ct 1, lo ct 0, lo ct 1
      if (abl & 256) return;   // (256: no MFMAs)
      acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, k < 2 ? pbl : pbh, acc[ct], 0, 0, 0);
    };
    request_corners(0, C[0]);
    request_weights(0, A[0]);
    request_weights(1, A[1]);
#pragma unroll
    for (int st = 0; st < 36; ++st) {
      f4t (&c)[8] = C[st & 1];
      f4t (&aw)[4] = A[(st + 1) & 1];    // the fragments of step st - 1
      // (in order: ... corners(st) [global part, if any], weights(st); both weight requests of the prologue are younger than corners(0),
      //  corners(1) is the youngest request at step 1)
      if (st == 0) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" : DW_THROUGH(c, aw));
      else if (st == 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : DW_THROUGH(c, aw));
      else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" : DW_THROUGH(c, aw));
      if (st + 1 < 36) request_corners(st + 1, C[(st + 1) & 1]);
      auto mfma = [&](int k) {
        if (st > 0) mfma_k(k, aw);
      };
      const float4 w = cw[st >> 2];
      dbf16x8 bh, bl;
      if (abl & 128) {   // (128: no blend / split arithmetic -- the MFMAs' B operands are raw corner bytes)
#pragma unroll
        for (int k = 0; k < 6; ++k) mfma(k);
        pbh = __builtin_bit_cast(dbf16x8, c[0]);
        pbl = __builtin_bit_cast(dbf16x8, c[1]);
        if (st >= 1 && st + 1 < 36) request_weights(st + 1, A[(st + 1) & 1]);
        continue;
      }
      // SCALAR fp32 instructions, written as asm: v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 -- what hipcc makes of this arithmetic,
      // two channels per instruction -- do NOT run under a wavefront's own MFMAs: 8 MFMAs + 64 packed FMAs take 256 + 336 cycles, with
      // v_fma_f32 (or conversions, integer instructions) 256 + 64 (tools/experiments/ubench/mfma_valu_overlap.hip).  Volatile asm keeps
      // its order: every channel's operation k before any channel's operation k + 1; the fences pin MFMA k between two stages.
      float e[8];   // the eight channels of the step: channel 4 (k >> 2) .. of piece (k >> 2), element k & 3
#define DW_FENCE asm volatile("" : "+v"(pbh), "+v"(pbl))
#define DW_CH(q, k) c[q + (k >> 2)][k & 3]   /* corner q / 2, channel k of the eight */
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(e[k]) : "v"(w.y), "v"(DW_CH(2, k)));
      DW_FENCE;
      mfma(0);
      DW_FENCE;
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(e[k]) : "v"(w.x), "v"(DW_CH(0, k)));
      DW_FENCE;
      mfma(1);
      DW_FENCE;
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(e[k]) : "v"(w.z), "v"(DW_CH(4, k)));
      DW_FENCE;
      mfma(2);
      DW_FENCE;
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(e[k]) : "v"(w.w), "v"(DW_CH(6, k)));
      DW_FENCE;
      mfma(3);
      DW_FENCE;
      unsigned hp[4], lp[4];   // hi / lo halves, two channels per register
#pragma unroll
      for (int k = 0; k < 4; ++k) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(hp[k]) : "v"(e[2 * k]), "v"(e[2 * k + 1]));
      DW_FENCE;
      mfma(4);
      DW_FENCE;
      float hf[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(hf[2 * k]) : "v"(hp[k]));
        asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(hf[2 * k + 1]) : "v"(hp[k]));
      }
      DW_FENCE;
      mfma(5);
      DW_FENCE;
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(e[k]) : "v"(hf[k]));
#pragma unroll
      for (int k = 0; k < 4; ++k) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(lp[k]) : "v"(e[2 * k]), "v"(e[2 * k + 1]));
#undef DW_FENCE
#undef DW_CH
      typedef unsigned u4t __attribute__((ext_vector_type(4)));
      bh = __builtin_bit_cast(dbf16x8, (u4t){hp[0], hp[1], hp[2], hp[3]});
      bl = __builtin_bit_cast(dbf16x8, (u4t){lp[0], lp[1], lp[2], lp[3]});
      pbh = bh;
      pbl = bl;
      if (st >= 1 && st + 1 < 36) request_weights(st + 1, A[(st + 1) & 1]);   // (into the registers step st - 1's MFMAs have just read)
    }
    {  // step 35's MFMAs
      f4t (&aw)[4] = A[1];
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(aw[0]), "+v"(aw[1]), "+v"(aw[2]), "+v"(aw[3]));
#pragma unroll
      for (int k = 0; k < 6; ++k) mfma_k(k, aw);
    }
#undef DW_THROUGH
#undef DW_LDS_READS
#undef DW_LDS_OFFS
  }
  // ---- epilogue: bias, LeakyReLU; the channels-last output leaves through LDS (round 6): from its accumulator layout a lane holds
  // 16-byte runs of a pixel's 256 bytes -- eight store instructions each touching 32 pixels with 32 bytes; a wavefront's 32 x 64 tile,
  // transposed through the (now free) window, leaves as whole 256-byte pixels, four per instruction ----
  if (abl & 8) return;
  float v[2][16];   // (all bias loads before the first store: see DF_EPILOGUE64_VALUES)
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) DF_EPILOGUE64_VALUES(v[ct], acc[ct], ct, kg, bias, act, slope)
  if (y && valid) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) DF_EPILOGUE64_STORE_Y(v[ct], ct, kg, y, (long)n * 64 * plane + p, plane)
  }
  if (yt) {
    __syncthreads();   // every wavefront has finished reading the window
    float* T = reinterpret_cast<float*>(win) + wave * (32 * 68);   // [pixel j][64 channels (+ 4: rows 272 bytes apart)]
    const int jj = lane & 31;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        *reinterpret_cast<float4*>(T + jj * 68 + ct * 32 + 8 * gq + 4 * kg) =
            make_float4(v[ct][4 * gq], v[ct][4 * gq + 1], v[ct][4 * gq + 2], v[ct][4 * gq + 3]);
    // (a wavefront reads back only what it wrote itself: no barrier)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int pj = 4 * it + (lane >> 4), part = lane & 15;
      int pg_, pi_;
      dw_patch_of(pj, pg_, pi_);
      const int pa = ty * DW_T + 2 * wave + pg_, pb_ = tx * DW_T + pi_;
      if (pa < H && pb_ < W)
        *reinterpret_cast<float4*>(yt + ((long)n * plane + (long)pa * W + pb_) * 64 + 4 * part) = *reinterpret_cast<const float4*>(T + pj * 68 + 4 * part);
    }
  }
}

}  // namespace

// Plane limits of the two LDS-window kernels (deform_conv64_fusedw_kernel, deform_conv64_x3w_kernel): a lane whose sample leaves the
// window reads its corners at 32-bit byte offsets from the image's first pixel (256 bytes per pixel: H * W < 2^24), and a tap's top-left
// corner travels packed as (y0 + 2) << 16 | (x0 + 2) with y0 <= H and x0 <= W (H + 2 < 2^15, W + 2 < 2^16).  Past any of them the
// launchers take the gathering kernels (64-bit offsets, the same bits); a caller that forces a window kernel there is refused.
// (DBM_DEFORM_WINDOW_LIMITS, deform_window.h, says the same in words)
bool deform_window_plane_ok(int H, int W) { return 256L * H * W < (1L << 32) && H <= 32765 && W <= 65533; }

void launch_deform_conv64_fusedw(const float* xt, const float* off, const float* wf, const float* bias, float* y, float* yt, int N, int H, int W,
                                 long offsn, int act, float slope, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    DBM_HIP(hipFuncSetAttribute((const void*)deform_conv64_fusedw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  const int tpi = (H * W + DWF_POS - 1) / DWF_POS;
  hipLaunchKernelGGL(deform_conv64_fusedw_kernel, dim3((unsigned)(N * tpi)), dim3(256), DWF_LDS, s, xt, off, wf, bias, y, yt, N, H, W, offsn, act,
                     slope, tpi, DBM_MEASURE_ENV("FUSEDW_ABL"));
}

void launch_deform_conv64_x3w(const float* xt, const float* off, const void* wx, const float* bias, float* y, float* yt, int N, int H, int W,
                              long offsn, int act, float slope, int tilesX, int tilesY, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    DBM_HIP(hipFuncSetAttribute((const void*)deform_conv64_x3w_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  hipLaunchKernelGGL(deform_conv64_x3w_kernel, dim3((unsigned)((long)N * tilesX * tilesY)), dim3(512), DW_LDS, s, xt, off, (const dbf16x8*)wx, bias,
                     y, yt, N, H, W, offsn, act, slope, tilesX, tilesY, DBM_MEASURE_ENV("X3W_ABL"));
}
