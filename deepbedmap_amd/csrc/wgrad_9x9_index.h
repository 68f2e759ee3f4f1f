// Index arithmetic of wgrad_wave_dma_9x9_kernel (wgrad.hip): LDS layout, read offsets, and which lane halves of a
// (step, tap) see a cell inside the plane.  Plain constexpr C++ (no HIP header): the kernel uses these functions, and
// tools/wgrad_9x9_index_check.cpp replays the loop with them on a CPU array laid out as the LDS is.
//
// A band is one 9 x 9 image.  Step s of the K loop feeds positions 2 s (lanes with kh = 0) and 2 s + 1 (kh = 1) to nine
// v_mfma_f32_32x32x2_f32, one per tap t = 3 ty + tx; the kh = 1 half of the last step is the padding position 81.  The x tile is an
// unframed slab [channel][81], so tap (ty, tx) of position q reads x[q + 9 (ty - 1) + (tx - 1)]: a cell of the neighbouring row or
// plane where the tap leaves the plane.  That value is finite but wrong, and it is multiplied by an A value read from a zero region
// in place of the dy slab.  An MFMA whose two halves are both outside is not issued.
#pragma once

namespace wgrad9 {

constexpr int H = 9, W = 9, T = 9;
constexpr int PLANE = H * W;              // 81
constexpr int SLAB = 32 * PLANE;          // floats of 32 planes: the dy slab, and one wavefront's x slab
constexpr int STEPS = (PLANE + 1) / 2;    // 41

// which lane halves of (step, tap) multiply a cell inside the plane; the value indexes the A operand set of a step
enum Valid { NONE = 0, KH0 = 1, KH1 = 2, BOTH = 3 };

constexpr bool tap_inside(int q, int t) {
  if (q >= PLANE) return false;           // the padding position
  const int r = q / W + t / 3 - 1, c = q % W + t % 3 - 1;
  return r >= 0 && r < H && c >= 0 && c < W;
}
constexpr int valid(int s, int t) { return (tap_inside(2 * s, t) ? KH0 : 0) | (tap_inside(2 * s + 1, t) ? KH1 : 0); }
constexpr bool step_uses(int s, int v) {  // does any tap of step s take the A operand of kind v?
  for (int t = 0; t < T; ++t)
    if (valid(s, t) == v) return true;
  return false;
}
constexpr int step_mfmas(int s) {
  int n = 0;
  for (int t = 0; t < T; ++t) n += valid(s, t) != NONE;
  return n;
}
constexpr int band_mfmas() {
  int n = 0;
  for (int s = 0; s < STEPS; ++s) n += step_mfmas(s);
  return n;
}

// LDS layout in floats.  Everything up to LDS_FLOATS is zeroed at kernel start; the guard and the zero region are never written again.
constexpr int LDS_Y = 0;                        // dy slab [32][81], shared by the two wavefronts
constexpr int LDS_GUARD = LDS_Y + SLAB;         // 4 zeros: the cell in front of plane 0 of wavefront 0's x slab
constexpr int LDS_X0 = LDS_GUARD + 4;           // x slabs [2][32][81], 16-byte aligned for 16-byte DMA
constexpr int LDS_ZERO = LDS_X0 + 2 * SLAB;     // zero region: A values of the halves outside the plane, the cell behind plane 31
constexpr int ZERO_FLOATS = 84;
constexpr int LDS_FLOATS = LDS_ZERO + ZERO_FLOATS;
constexpr int lds_x(int wave) { return LDS_X0 + wave * SLAB; }

// A reads: base[a_off(s)], one read per kind of validity that the step uses.  Lane (j, kh):
//   BOTH: base = dy plane j + kh;   KH0: kh = 0 the same, kh = 1 the zero region;   KH1: kh = 1 the same, kh = 0 the zero region
constexpr int a_off(int s) { return 2 * s; }
constexpr int a_base(int v, int j, int kh) { return ((v >> kh) & 1) ? LDS_Y + j * PLANE + kh : LDS_ZERO; }
// B reads: base[b_off(s, t)] with base = x plane j of the wavefront's slab - B_BACK + kh, for every tap whose MFMA is issued
constexpr int B_BACK = W + 1;
constexpr int b_off(int s, int t) { return 2 * s + (t / 3) * W + t % 3; }
constexpr int b_base(int wave, int j, int kh) { return lds_x(wave) + j * PLANE - B_BACK + kh; }

constexpr int max_b_off() {
  int m = 0;
  for (int s = 0; s < STEPS; ++s)
    for (int t = 0; t < T; ++t)
      if (valid(s, t) != NONE && b_off(s, t) > m) m = b_off(s, t);
  return m;
}

// 12 in steps 0-3 (ty = 0 above row 0), 12 in steps 36-39 (ty = 2 below row 8), 5 in step 40 (position 80 with ty = 2 or tx = 2 beside
// the padding position), and tap (0, 0) of step 4: position 8 = (0, 8) has no row above, position 9 = (1, 0) no column to the left
static_assert(band_mfmas() == STEPS * T - 30, "MFMAs per band");
static_assert(band_mfmas() == 339, "MFMAs per band");
static_assert(step_mfmas(0) == 6 && step_mfmas(4) == 8 && step_mfmas(5) == 9 && step_mfmas(36) == 6 && step_mfmas(STEPS - 1) == 4, "MFMAs per step");
static_assert(a_off(STEPS - 1) < ZERO_FLOATS, "the zero region holds every A offset");
static_assert(max_b_off() < 256, "B offsets fit the 8-bit dword fields of ds_read2_b32");
static_assert(LDS_X0 % 4 == 0 && SLAB % 4 == 0, "16-byte DMA lands on 16-byte-aligned LDS");
static_assert(STEPS % 2 == 1, "the unrolled loop ends on the first operand set");

}  // namespace wgrad9
