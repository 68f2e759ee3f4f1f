// Planner of the batched weight gradients (wgrad.hip): everything that is decided without touching the device.  Host-only: plain
// C++17, no HIP header, no HIP call (tools/wgrad_plan_check.cpp compiles it alone and pins its results).
//
//   wgrad_layout(descriptors, deterministic, cleared_target) -> WgradLayout
//
// picks a kernel form per descriptor (WGRAD_FORMS below), plans every form's launch (band shapes, K split, workgroup prefix table)
// and lays out the pair buffers of the deterministic folding as float offsets into one arena per form.  WgradBatch::build() only
// allocates, turns the offsets into pointers and uploads.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#ifndef DBM_CHECK  // (stand-alone use; the library's own DBM_CHECK throws DbmError)
#include <stdexcept>
#include <string>
#define DBM_CHECK(cond, msg)                                                \
  do {                                                                      \
    if (!(cond)) throw std::runtime_error(std::string(msg) + " (" #cond ")"); \
  } while (0)
#endif

// gW[o][c][ky][kx] (+)= scale * sum_{n,a,b} dy[n][o][a][b] * x[n][c][(a*stride+ky-pad)>>ups][...]
struct WgradDesc {
  const float* x;   // input activations
  long xsn; int xsc; int Cin; int Hin, Win; int ups;
  const float* dy;  // output gradients
  long dysn; int dysc; int Cout; int OH, OW;
  int KH, KW, stride, pad;
  int N;
  float scale;
  float* gW;        // canonical OIHW, accumulated with atomicAdd
  float* gb;        // may be null; accumulated with atomicAdd
};

struct WgradPlan {
  WgradDesc d;
  int groups, coutTiles, S;  // workgroups = groups (input-channel groups) x coutTiles x S (K splits)
  int wg_count;
  int G;        // 32-channel input tiles per workgroup (= active wavefronts)
  int IB, R;    // band = IB images x R output rows
  int nbr;      // row-bands per image
  int BP, BPp;  // positions per band, padded to even
  int YS;       // LDS row stride of the dy slab (odd)
  int Rin, Wst; // staged logical input patch rows / cols per image (direct form: Wst = segments per output row)
  int ImgS;     // Rin*Wst
  int XS;       // LDS channel stride of the patch (odd)
  int nbands;   // (direct form: segments of 8 positions; 1x1 GEMM form: bands of 32 positions)
  // whole-image bands of plain (not upsampled) planes: both operands are contiguous per image and are staged with
  // 16-byte loads; `fast` = 0 falls back to the per-element gather
  int fast;
  unsigned planeM, winM;  // ceil(2^32 / (Hin*Win)), ceil(2^32 / Win): exact quotients for the sizes staged here
  int layout0[2];         // (unused: keeps the fields behind it where the kernels were measured -- see `layout1`)
  const float* zeros;     // >= 4 bytes of device zeros (out-of-image rows of the row-band DMA form); set by WgradBatch::build
  // Slot partials: partial[slice][cout tile][group][slot][tap][16][64] in accumulator order, partial_b[slice][cout tile][32].  The planner
  // always leaves them null (deterministic mode folds through the pair buffers below).  The kernels' epilogue for them stays: without
  // its three branches wgrad_band_dma_kernel<16,8> and wgrad_kernel<1,1> measured slower than the parent's own run-to-run range
  // (profiles/r7/wgrad_forms_refactor.txt, 4a, has the registers and times).
  float* partial;
  float* partial_b;
  // layout0 / layout1 / layout2 hold the places of fields no kernel reads any more (oplaneM, wave_task; fold_start; three fold-table
  // ints).  They are padding with a measured reason: without them the struct is 256 instead of 280 bytes and every field behind winM
  // moves; with the kernels' text otherwise the parent's, wgrad_band_dma_kernel<16,8> then took 155.6 against 154.0 us standalone and
  // wgrad_wave_dma_kernel 356.2 against 354.2, both outside the parent's run-to-run range; with the padding 156.2 against 156.1 and
  // 363.6 against 364.1 (profiles/r7/wgrad_forms_refactor.txt, 5 and 6).  Keep offsets and size when fields come or go.
  int layout1;
  int fold_slots;
  int layout2[3];
  // Pair buffers (deterministic folding, no fp32 atomics on the K split): K slices 2k and 2k + 1 add with atomics into buffer k, which is
  // zero and has gW's own layout (+ Cout bias floats): two contributions commute bit for bit.  pair_direct: pair 0 goes
  // straight to gW / gb (the gradient is known to be zero).  wgrad_pair_fold_kernel adds the buffers in order, clears them.
  float* pairW;       // set by WgradBatch::build from WgradFormLayout::pair_off
  long pair_stride;   // floats per buffer: Cout * Cin * T, then Cout
  int pair_n, pair_direct;
  // Several descriptors of one launch that add into the SAME gradient (the real- and the fake-batch graph of the discriminator): all of
  // them go through pair buffers (also a single slice, never pair_direct), the first one's fold job adds every member's buffer sum
  // -- this plan's, then plans[pair_next]'s, ... -- and updates the gradient ONCE per element: g + (a + b), whatever g holds and
  // whoever finishes first.  (Two fold jobs adding a and b with atomics gave (g + a) + b or (g + b) + a: reproducible only for g = 0.)
  int pair_next;      // next plan of the same category that shares this gradient (-1: none)
};

// wgrad_s2tiny_kernel's plan (4x4 stride 2 / 3x3 stride 1 layers on planes of <= 4 x 4; described at the kernel)
struct TinyPlan {
  const float* x[2];    // input activations of the (up to two) graphs; x[1] == null: one graph
  const float* dy[2];
  float* gW;
  long xsn, dysn;
  int N, Cin, Cout, Hin, Win, OH, OW;
  float scale;
  int wg_start, ctiles;  // workgroups of this layer: (Cout / 16) * ctiles, ctiles = Cin / 16
  int K;                 // 4: 4x4 stride 2 pad 1;  3: 3x3 stride 1 pad 1 (round 3: conv_layer6 / 8 of the discriminator)
};
constexpr int TINY_MAXK = 2048;  // K entries (images x valid output positions) a kernel row may have: 64 KB of LDS tables

// How a form's launch splits K (the position axis).  The plan functions take the outcome as a WgradSplit.
enum class WgradKSplit {
  Level,  // workgroup forms: positions per workgroup halved (`level` 0 .. 3) until the launch offers enough workgroups
  Slots,  // LDS-DMA forms: S = slots / units, ONE round of equally long two-wavefront groups over the chip
  Work,   // 1x1 GEMM and direct forms: equally long workgroups of work / 512 K segments, at least `kparam`
};
struct WgradSplit {
  int level = 0;           // Level
  int S_fixed = 0;         // Slots (0: the form's own rule, 648 positions per workgroup)
  long per_wg = 1L << 40;  // Work: K segments one workgroup works through
};
typedef size_t (*WgradPlanFn)(const WgradDesc& d, WgradPlan& p, const WgradSplit& k);  // fills p -> dynamic LDS bytes, 0: not eligible

inline int odd_up(int v) { return v | 1; }

inline void plan_begin(const WgradDesc& d, WgradPlan& p) {
  memset(&p, 0, sizeof(p));
  p.d = d;
  p.pair_next = -1;
}

// ---- forms that stage bands of whole images (workgroup forms, wave-DMA form) ----
inline void check_kernel_size(const WgradDesc& d) {
  const int T = d.KH * d.KW;
  DBM_CHECK(T == 1 || T == 9 || T == 16, "wgrad: supported kernels are 1x1, 3x3, 4x4");
  DBM_CHECK(d.OW < 4096 && d.OH < 4096, "wgrad: image too large");
}

// whole-image bands: images per band, doubled while the band stays within `budget` floats of LDS
template <class Cost>
inline int images_per_band(const WgradDesc& d, int level, long budget, Cost cost) {
  int IB = 1;
  while (IB * 2 <= d.N && IB * 2 <= 128 && IB * 2 * d.OH * d.OW <= (324 >> std::max(level, 0)) && cost(IB * 2, d.OH) <= budget) IB *= 2;
  return IB;
}

// band = IB images x R output rows (groups / G / coutTiles are set): strides, K split and the 16-byte staging flag
inline void plan_bands(const WgradDesc& d, WgradPlan& p, int IB, int R, const WgradSplit& k) {
  p.IB = IB; p.R = R;
  p.nbr = (d.OH + R - 1) / R;
  p.BP = IB * R * d.OW;
  p.BPp = (p.BP + 1) & ~1;
  p.YS = odd_up(p.BPp);
  p.Rin = (R - 1) * d.stride + d.KH;
  p.Wst = (d.OW - 1) * d.stride + d.KW;
  p.ImgS = p.Rin * p.Wst;
  p.XS = odd_up(IB * p.ImgS);
  DBM_CHECK(p.Rin < 4096 && p.Wst < 4096, "wgrad: patch too large");
  const int imgGroups = (d.N + IB - 1) / IB;
  p.nbands = imgGroups * p.nbr;
  // K split: enough positions per workgroup that the closing atomics stay a small fraction of the MFMA work
  // (~8 images of the 9x9 trunk per workgroup; `level` > 0 halves that, and the band, per step: used by batches
  // that would otherwise leave most of the chip idle)
  const long positions = (long)d.N * d.OH * d.OW;
  const long per_wg = k.level >= 0 ? std::max(1L, 648L >> k.level) : (648L << -k.level);
  int S = (int)((positions + per_wg - 1) / per_wg);
  if (k.S_fixed > 0) S = k.S_fixed;
  if (S > p.nbands) S = p.nbands;
  if (S < 1) S = 1;
  p.S = S;
  p.wg_count = p.groups * p.coutTiles * S;
  auto magic = [](unsigned dv) { return (unsigned)((0x100000000ULL + dv - 1) / dv); };
  const int plane = d.Hin * d.Win, oplane = d.OH * d.OW;
  p.planeM = magic((unsigned)plane);
  p.winM = magic((unsigned)d.Win);
  // contiguous 16-byte staging: whole-image bands of plain planes, every per-image run 16-byte aligned and a
  // multiple of four floats (all channel counts of a run: full tiles / groups and the ragged last one)
  const int chx = p.G * 32;
  const int tail_ci = d.Cin - (p.groups - 1) * chx, tail_co = d.Cout - (p.coutTiles - 1) * 32;
  auto mult4 = [](long v) { return (v % 4) == 0; };
  // (d.Win > 1: the multiply-high constants ceil(2^32 / dv) do not exist for dv = 1 -- a plane one pixel wide, e.g. the 1x1
  // view of the input block's k6 s2 branch on 3 x 3 tiles, got every sample of a run decoded to channel 0; found by the
  // randomised-geometry tests of round 3)
  p.fast = d.Win > 1 && p.nbr == 1 && d.ups == 0 && d.xsc == plane && d.dysc == oplane && mult4(d.xsn) && mult4(d.dysn) &&
           ((uintptr_t)d.x % 16) == 0 && ((uintptr_t)d.dy % 16) == 0 && mult4(32L * oplane) && mult4((long)chx * plane) &&
           mult4((long)std::min(32, tail_co) * oplane) && mult4((long)std::min(chx, tail_ci) * plane) &&
           (long)chx * plane < (1L << 20) && 32L * oplane < (1L << 20) && plane < 4096 && oplane < 4096;
}

// workgroup forms (wgrad_kernel<T, TPW>): every layer the other forms refuse.  Whole images per band if small, else row bands.
inline size_t plan_workgroup(const WgradDesc& d, WgradPlan& p, const WgradSplit& k) {
  check_kernel_size(d);
  plan_begin(d, p);
  const int T = d.KH * d.KW;
  const int tiles = (d.Cin + 31) / 32;
  p.groups = (tiles + 3) / 4;
  p.G = (tiles + p.groups - 1) / p.groups;
  p.coutTiles = (d.Cout + 31) / 32;
  const int Wst = (d.OW - 1) * d.stride + d.KW;
  const long budget = (T <= 9) ? 19800 : 25000;  // floats: <= 79 KB lets two workgroups share a CU's 160 KB
  auto cost = [&](int IB, int R) {
    const int Rin = (R - 1) * d.stride + d.KH;
    const long bpp = (IB * R * d.OW + 1) & ~1;
    return (long)p.G * 32 * odd_up(IB * Rin * Wst) + 32L * odd_up((int)bpp) + 2 * bpp + (long)IB * Rin * Wst;
  };
  int IB = 1, R = d.OH;
  if (cost(1, d.OH) <= budget) IB = images_per_band(d, k.level, budget, cost);
  else while (R > 1 && cost(1, R) > budget) --R;
  DBM_CHECK(cost(IB, R) <= 38000, "wgrad: band does not fit in LDS");
  plan_bands(d, p, IB, R, k);
  const size_t stage = sizeof(float) * ((size_t)32 * p.YS + 2 * (size_t)p.BPp + (size_t)IB * p.ImgS + (size_t)p.G * 32 * p.XS);
  const size_t epilogue = sizeof(float) * 4 * 8 * 32 * (size_t)T;  // per-wavefront transpose areas
  return std::max(stage, epilogue);
}

// wave-DMA form (wgrad_wave_dma_kernel): 3x3 / stride 1 / pad 1 on small planes, whole-image bands only, 16-byte staging only
inline size_t plan_wave_dma(const WgradDesc& d, WgradPlan& p, const WgradSplit& k) {
  check_kernel_size(d);
  plan_begin(d, p);
  const int T = d.KH * d.KW;
  if (!(T == 9 && d.stride == 1 && d.pad == 1 && d.OH == d.Hin && d.OW == d.Win && (d.OH + 2) * (d.OW + 1) <= 128)) return 0;
  const int tiles = (d.Cin + 31) / 32;
  p.groups = (tiles + 1) / 2;
  p.G = 2;
  p.coutTiles = (d.Cout + 31) / 32;
  const long budget = 10000;  // floats: four two-wavefront groups per CU
  auto cost = [&](int IB, int R) {
    const long bpp = (IB * R * d.OW + 1) & ~1;
    return 32L * IB * d.OH * d.OW + 4 + 64L * IB * (d.OH + 2) * (d.OW + 1) + bpp + 8;
  };
  if (cost(1, d.OH) > budget) return 0;
  const int IB = images_per_band(d, k.level, budget, cost);
  plan_bands(d, p, IB, d.OH, k);
  const int oplane = d.OH * d.OW;
  if (!p.fast || (long)IB * 32 * oplane >= 65536 || (long)IB * 32 * (d.OH + 2) * (d.OW + 1) >= 32768) return 0;
  p.ImgS = (d.OH + 2) * (d.OW + 1);  // the framed plane
  const size_t stage = sizeof(float) * ((size_t)32 * IB * oplane + 4 + (size_t)64 * IB * p.ImgS + (size_t)p.BPp + 8);
  return std::max(stage, sizeof(float) * 2 * 8 * 32 * (size_t)T);
}

// row-band LDS-DMA form (wgrad_band_dma_kernel): the largest band of R output rows whose slabs fit half a CU's LDS
inline size_t plan_band_dma(const WgradDesc& d, WgradPlan& p, const WgradSplit& k) {
  check_kernel_size(d);
  plan_begin(d, p);
  const int T = d.KH * d.KW;
  if (!(T == 9 || T == 16) || d.KH != d.KW) return 0;
  const int tiles = (d.Cin + 31) / 32;
  p.groups = T == 9 ? (tiles + 1) / 2 : tiles;
  p.G = T == 9 ? 2 : 1;
  p.coutTiles = (d.Cout + 31) / 32;
  const int nx = T == 9 ? 2 : 1;
  const int Wl = d.Win << d.ups, Wf = Wl + 1;
  auto floats = [&](int R) {
    const int Rin = (R - 1) * d.stride + d.KH;
    const int bpp = (R * d.OW + 1) & ~1;
    return 32L * odd_up(bpp) + 4 + (long)nx * 32 * odd_up(Rin * Wf) + bpp + 8;
  };
  auto fits = [&](int R) {
    const int Rin = (R - 1) * d.stride + d.KH;
    return Rin * Wf <= 512 && R * d.OW <= 512 && floats(R) <= 19400 && (R * d.stride + d.KH) * Wf < 32768;
  };
  if (!fits(1) || d.OH * d.OW < 64) return 0;  // tiny planes: several images per band (workgroup / trunk forms)
  int R = 1;
  while (R < d.OH && fits(R + 1)) ++R;
  // equal bands: the smallest R with the same number of bands per image
  const int nbr = (d.OH + R - 1) / R;
  R = (d.OH + nbr - 1) / nbr;
  p.IB = 1; p.R = R; p.nbr = nbr;
  p.BP = R * d.OW;
  p.BPp = (p.BP + 1) & ~1;
  p.YS = odd_up(p.BPp);
  p.Rin = (R - 1) * d.stride + d.KH;
  p.Wst = Wf;
  p.ImgS = p.Rin * Wf;
  p.XS = odd_up(p.ImgS);
  p.nbands = d.N * nbr;
  p.S = std::min(k.S_fixed > 0 ? k.S_fixed : 1, p.nbands);
  p.wg_count = p.groups * p.coutTiles * p.S;
  const size_t stage = sizeof(float) * (size_t)floats(R);
  return std::max(stage, sizeof(float) * 2 * 8 * 32 * (size_t)9);
}

// direct form (wgrad_direct_kernel<MODE>): mode 0 / 1 / 2 or -1 if the layer is not eligible
inline int direct_mode(const WgradDesc& d) {
  const int T = d.KH * d.KW;
  const int Hl = d.Hin << d.ups, Wl = d.Win << d.ups;
  if (d.KH != d.KW || d.pad != 1 || d.OW < 16 || d.xsc != d.Hin * d.Win || d.dysc != d.OH * d.OW) return -1;
  if (T == 9 && d.stride == 1 && d.OH == Hl && d.OW == Wl) return d.ups ? 1 : 0;
  if (T == 16 && d.stride == 2 && d.ups == 0 && 2 * d.OH == Hl && 2 * d.OW == Wl) return 2;
  return -1;
}

// k.per_wg: K segments (8 positions each) one workgroup (four wavefronts) works through
template <int MODE>
inline size_t plan_direct(const WgradDesc& d, WgradPlan& p, const WgradSplit& k) {
  if (direct_mode(d) != MODE) return 0;
  plan_begin(d, p);
  const int T = d.KH * d.KW;
  p.groups = (d.Cin + 31) / 32;
  p.G = 1;
  p.coutTiles = (d.Cout + 31) / 32;
  p.Wst = (d.OW + 7) / 8;
  const long nseg = (long)d.N * d.OH * p.Wst;
  DBM_CHECK(nseg < (1L << 30), "wgrad: too many positions");
  p.nbands = (int)nseg;
  p.S = (int)std::max(1L, (nseg + k.per_wg - 1) / k.per_wg);
  p.wg_count = p.groups * p.coutTiles * (MODE == 2 ? 2 : 1) * p.S;
  p.IB = 1; p.R = 1; p.nbr = d.OH; p.BP = p.BPp = 8;
  return sizeof(float) * 4 * 8 * 32 * (size_t)T;  // four transpose areas of 8 output rows
}

// 1x1 layers on large contiguous planes (wgrad_1x1_kernel); k.per_wg: bands of 32 positions per workgroup
inline size_t plan_gemm1x1(const WgradDesc& d, WgradPlan& p, const WgradSplit& k) {
  const int plane = d.OH * d.OW;
  if (!(d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0 && d.ups == 0 && d.Hin == d.OH && d.Win == d.OW && plane >= 256 &&
        plane % 4 == 0 && d.xsc == plane && d.dysc == plane && d.xsn % 4 == 0 && d.dysn % 4 == 0 &&
        ((uintptr_t)d.x % 16) == 0 && ((uintptr_t)d.dy % 16) == 0))
    return 0;
  plan_begin(d, p);
  p.groups = (d.Cin + 127) / 128;
  p.G = 4;
  p.coutTiles = (d.Cout + 63) / 64;
  p.nbr = (plane + 31) / 32;
  p.nbands = d.N * p.nbr;
  p.S = (int)std::max(1L, (p.nbands + k.per_wg - 1) / k.per_wg);
  p.wg_count = p.groups * p.coutTiles * p.S;
  p.IB = 1; p.R = 1; p.BP = p.BPp = 32; p.YS = p.XS = 36;
  return sizeof(float) * 2 * (64 + 128) * 36;
}

// ---------------------------------------------------------------------------------------------------------------
// THE form table: one row per category, in the numbering tests, tools and profiles/ use.
//   X(category, profiler tag, taps, kernel, threads per workgroup, dynamic-LDS attribute, plan function, K split, kparam)
// kparam: Slots -- the slot count of launches of <= 32 units (0: no such rule);  Work -- the least K segments per workgroup.
// The kernel column is read by wgrad.hip only (the launch), the others by the planner below.
// ---------------------------------------------------------------------------------------------------------------
#define WGRAD_FORMS(X)                                                                                                    \
  X(0, "wgrad<1,1>",     1,  (wgrad_kernel<1, 1>),           256, 156 * 1024, plan_workgroup, WgradKSplit::Level, 0)      \
  X(1, "wgrad<9,9>",     9,  (wgrad_kernel<9, 9>),           256, 156 * 1024, plan_workgroup, WgradKSplit::Level, 0)      \
  X(2, "wgrad<16,8>",    16, (wgrad_kernel<16, 8>),          512, 156 * 1024, plan_workgroup, WgradKSplit::Level, 0)      \
  X(3, "wave_dma",       9,  (wgrad_wave_dma_kernel),        128, 100 * 1024, plan_wave_dma,  WgradKSplit::Slots, 256)    \
  X(4, "band_dma<9,9>",  9,  (wgrad_band_dma_kernel<9, 9>),  128, 100 * 1024, plan_band_dma,  WgradKSplit::Slots, 0)      \
  X(5, "band_dma<16,8>", 16, (wgrad_band_dma_kernel<16, 8>), 128, 100 * 1024, plan_band_dma,  WgradKSplit::Slots, 0)      \
  X(6, "direct<0>",      9,  (wgrad_direct_kernel<0>),       256, 72 * 1024,  plan_direct<0>, WgradKSplit::Work,  64)     \
  X(7, "direct<1>",      9,  (wgrad_direct_kernel<1>),       256, 72 * 1024,  plan_direct<1>, WgradKSplit::Work,  64)     \
  X(8, "direct<2>",      16, (wgrad_direct_kernel<2>),       256, 72 * 1024,  plan_direct<2>, WgradKSplit::Work,  64)     \
  X(9, "wgrad_1x1",      1,  (wgrad_1x1_kernel),             256, 72 * 1024,  plan_gemm1x1,   WgradKSplit::Work,  8)

constexpr int WGRAD_NCAT = 10;
struct WgradForm {
  const char* tag;
  int T, threads, lds_attr;
  WgradPlanFn plan;
  WgradKSplit ksplit;
  int kparam;
};
#define WGRAD_FORM_ROW(cat, tag, T, kernel, threads, lds_attr, plan, ksplit, kparam) {tag, T, threads, lds_attr, plan, ksplit, kparam},
inline const WgradForm kWgradForms[WGRAD_NCAT] = {WGRAD_FORMS(WGRAD_FORM_ROW)};
#undef WGRAD_FORM_ROW

// Order of preference per tap count: the first form whose plan function accepts the layer (the workgroup forms accept all).
inline const int kPrefer3x3[] = {3, 6, 7, 4, 1, -1};  // wave_dma, direct (plain / on a nearest-x2 input), band_dma, workgroup
inline const int kPrefer4x4[] = {8, 5, 2, -1};        // direct, band_dma, workgroup
inline const int kPrefer1x1[] = {9, 0, -1};           // 1x1 GEMM, workgroup

inline int choose_form(const WgradDesc& d) {
  const int T = d.KH * d.KW;
  const int* pref = T == 1 ? kPrefer1x1 : T == 9 ? kPrefer3x3 : kPrefer4x4;  // (other sizes: refused by the 4x4 list's checks)
  WgradPlan p;
  for (; *pref >= 0; ++pref)
    if (kWgradForms[*pref].plan(d, p, WgradSplit()) != 0) return *pref;
  DBM_CHECK(false, "wgrad: no form accepts the layer (every list ends with a workgroup form, which accepts all)");
  return -1;
}

struct WgradFormLayout {
  std::vector<WgradPlan> plans;  // zeros and pairW are null
  std::vector<long> pair_off;    // per plan: float offset of its pair buffers in the form's arena (-1: none)
  std::vector<int> starts;       // prefix table of the launch (plans + 1 entries); deterministic: the fold starts (plans entries) behind it
  int total_wg = 0, fold_wgs = 0;
  size_t lds = 0;
  size_t arena_floats = 0;       // pair-buffer arena to allocate and clear (0: none)
  double flops = 0.0, abytes = 0.0;  // abytes: algorithmic bytes of the launch, every layer's x, dy and gW once
};

struct WgradLayout {
  WgradFormLayout form[WGRAD_NCAT];
  std::vector<TinyPlan> tiny;
  int tiny_wgs = 0, tiny_rowlen = 4;
  double tiny_flops = 0.0, tiny_bytes = 0.0;
  std::vector<int> tiny_owner;       // per descriptor: its tiny plan, -1: none
  std::vector<int> desc_cat, desc_S; // per descriptor: category (-1: wgrad_s2tiny_kernel) and K slices S (tiny: 1)
};

inline bool s2tiny_eligible(const WgradDesc& d) {
  const bool k4 = d.KH == 4 && d.KW == 4 && d.stride == 2;
  const bool k3 = d.KH == 3 && d.KW == 3 && d.stride == 1 && d.Hin == d.OH && d.Win == d.OW;
  return (k4 || k3) && d.pad == 1 && d.ups == 0 && d.OW <= 4 && d.OH <= 4 && d.gb == nullptr &&
         d.Cin % 32 == 0 && d.Cout % 32 == 0 && d.xsc == d.Hin * d.Win && d.dysc == d.OH * d.OW && d.Win >= 2 &&
         (long)d.N * d.OH * d.OW + 4 <= TINY_MAXK && (long)d.N * d.xsn < (1L << 31) && (long)d.N * d.dysn < (1L << 27);
}

// Layers on tiny planes: their own kernel (wgrad_s2tiny_kernel), outside the form table.  Two descriptors with the same gradient
// (the real- and the fake-batch graph of the discriminator) share a plan.
inline void plan_tiny(const std::vector<WgradDesc>& descs, WgradLayout& L) {
  L.tiny_owner.assign(descs.size(), -1);
  for (size_t i = 0; i < descs.size(); ++i) {
    if (L.tiny_owner[i] >= 0) continue;
    const WgradDesc& d = descs[i];
    // the descriptors that add to this gradient: all of them must qualify, at most two, same geometry
    std::vector<size_t> grp;
    bool ok = true;
    for (size_t k = 0; k < descs.size(); ++k) {
      if (descs[k].gW != d.gW) continue;
      const WgradDesc& f = descs[k];
      grp.push_back(k);
      ok = ok && s2tiny_eligible(f) && f.KH == d.KH && f.N == d.N && f.Cin == d.Cin && f.Cout == d.Cout && f.Hin == d.Hin && f.Win == d.Win &&
           f.OH == d.OH && f.OW == d.OW && f.xsn == d.xsn && f.dysn == d.dysn && f.scale == d.scale;
    }
    if (!ok || grp.size() > 2 || grp[0] != i) continue;
    TinyPlan q;
    memset(&q, 0, sizeof(q));
    for (size_t u = 0; u < grp.size(); ++u) { q.x[u] = descs[grp[u]].x; q.dy[u] = descs[grp[u]].dy; L.tiny_owner[grp[u]] = (int)L.tiny.size(); }
    q.gW = d.gW; q.xsn = d.xsn; q.dysn = d.dysn;
    q.N = d.N; q.Cin = d.Cin; q.Cout = d.Cout; q.Hin = d.Hin; q.Win = d.Win; q.OH = d.OH; q.OW = d.OW; q.scale = d.scale;
    q.ctiles = d.Cin / 16; q.wg_start = L.tiny_wgs; q.K = d.KH;
    L.tiny_wgs += (d.Cout / 16) * q.ctiles;
    L.tiny.push_back(q);
    L.tiny_flops += 2.0 * (double)grp.size() * d.N * d.OH * d.OW * d.Cout * d.Cin * (d.KH * d.KW);
    L.tiny_bytes += 4.0 * ((double)grp.size() * d.N * ((double)d.Cin * d.Hin * d.Win + (double)d.Cout * d.OH * d.OW) + (double)d.Cout * d.Cin * (d.KH * d.KW));
    L.tiny_rowlen = std::max(L.tiny_rowlen, ((q.N * q.OH * q.OW + 3) / 4) * 4);
  }
}

// The K split of one form's launch over its layers `ds` (WgradKSplit)
inline WgradSplit split_policy(const WgradForm& f, const std::vector<WgradDesc>& ds) {
  WgradSplit k;
  if (f.ksplit == WgradKSplit::Level) return k;
  // one probe per layer at S = 1: LDS need, units (= workgroups of one K slice) and K segments of work
  WgradSplit one;
  one.S_fixed = 1;
  size_t need = 0;
  long units = 0, work = 0;
  for (const WgradDesc& d : ds) {
    WgradPlan p;
    need = std::max(need, f.plan(d, p, one));
    units += p.wg_count;
    work += (long)p.wg_count * p.nbands;
  }
  if (f.ksplit == WgradKSplit::Work) {
    // equally long workgroups, about two per CU over the whole launch (a workgroup's K range should stay long enough that its closing
    // atomics are a small fraction: direct form >= 64 segments = 512 positions; 1x1 GEMM >= 8 bands of 32 positions)
    k.per_wg = std::max((long)f.kparam, (work + 511) / 512);
    return k;
  }
  // LDS-DMA forms: the K split is chosen so that the launch is ONE round of equally long two-wavefront groups
  // (four per CU for the trunk form; two or four per CU for row bands, by their LDS footprint)
  // (few-layer launches -- the discriminator's conv_layer4: 16 units -- take a coarser K split: 256 workgroups of four images
  // instead of 1024 of one, a quarter of the partial tiles to write and fold: 116 -> 90 us standalone, round 3)
  int slots = need > 40 * 1024 ? 512 : 1024;
  // (<= 32 units: in data-parallel runs the trunk's launches are cut into four groups of 126 units each -- those keep the fine split)
  // (kparam is 0 for the row-band forms: they lose, 164 -> 204 us)
  if (f.kparam && units > 0 && units <= 32) slots = std::min(slots, f.kparam);
  if (units > 0) k.S_fixed = (int)std::max(1L, slots / units);
  return k;
}

// Pair buffers of a form's launch in deterministic mode: slices 2k, 2k + 1 -> buffer k (pair 0 straight to the gradient when it is
// known to be zero); plans that add into one gradient (same tensor, same geometry) are chained behind the first one
// (WgradPlan::pair_next).  Buffers are float offsets into one arena; the fold table rides behind the launch table.
inline void plan_pairs(WgradFormLayout& F, bool cleared_target) {
  std::vector<WgradPlan>& plans = F.plans;
  const int np = (int)plans.size();
  std::vector<int> first(np), shared(np, 0);
  for (int i = 0; i < np; ++i) {
    first[i] = i;
    for (int j = 0; j < i; ++j) {
      const WgradDesc &a = plans[j].d, &b = plans[i].d;
      if (a.gW == b.gW && a.gb == b.gb && a.Cout == b.Cout && a.Cin == b.Cin && a.KH == b.KH && a.KW == b.KW) { first[i] = first[j]; break; }
    }
    if (first[i] != i) shared[i] = shared[first[i]] = 1;
  }
  long off = 0;
  for (int i = 0; i < np; ++i) {
    WgradPlan& pl = plans[i];
    F.starts.push_back(F.fold_wgs);
    const int npair = (pl.S + 1) / 2;
    const int nb = shared[i] ? npair : pl.S > 1 ? std::max(0, npair - (cleared_target ? 1 : 0)) : 0;
    if (nb <= 0) continue;  // one slice, or two slices onto a cleared gradient: plain atomics commute
    // (the stride is the exact tensor size + bias; the arena offset is rounded up to four floats)
    pl.pair_stride = (long)pl.d.Cout * pl.d.Cin * pl.d.KH * pl.d.KW + pl.d.Cout;
    pl.pair_n = nb; pl.pair_direct = shared[i] ? 0 : (cleared_target ? 1 : 0);
    F.pair_off[i] = off;
    off += (long)nb * ((pl.pair_stride + 3) & ~3L);
    if (shared[i]) {
      for (int j = i + 1; j < np; ++j)
        if (first[j] == first[i]) { pl.pair_next = j; break; }
      if (first[i] != i) continue;  // folded by the first plan of its gradient: no fold workgroups of its own
    }
    F.fold_wgs += (int)((pl.pair_stride + 255) / 256);
  }
  F.arena_floats = (size_t)off + 4;
}

inline WgradLayout wgrad_layout(const std::vector<WgradDesc>& descs, bool deterministic, bool cleared_target) {
  WgradLayout L;
  plan_tiny(descs, L);
  L.desc_cat.assign(descs.size(), -1);
  L.desc_S.assign(descs.size(), 1);
  for (size_t i = 0; i < descs.size(); ++i)
    if (L.tiny_owner[i] < 0) L.desc_cat[i] = choose_form(descs[i]);
  for (int g = 0; g < WGRAD_NCAT; ++g) {
    const WgradForm& f = kWgradForms[g];
    WgradFormLayout& F = L.form[g];
    std::vector<WgradDesc> ds;
    for (size_t i = 0; i < descs.size(); ++i)
      if (L.desc_cat[i] == g) ds.push_back(descs[i]);
    if (ds.empty()) { F.starts.push_back(0); continue; }
    WgradSplit k = split_policy(f, ds);
    // workgroup forms: a launch should offer about two workgroups per CU; small batches split their position axis finer
    for (k.level = 0;; ++k.level) {
      F.plans.clear(); F.starts.clear();
      F.total_wg = 0; F.lds = 0;
      for (const WgradDesc& d : ds) {
        WgradPlan p;
        F.lds = std::max(F.lds, f.plan(d, p, k));
        F.starts.push_back(F.total_wg);
        F.total_wg += p.wg_count;
        F.plans.push_back(p);
      }
      // (deterministic mode: no finer K split than necessary -- every extra slice is a pair buffer to write and fold --
      // but a launch of a few dozen workgroups, e.g. the 4x4 layers of the deep discriminator, is split as well)
      // (256 since round 5 -- the input block's GEMM-shaped launch, 144 workgroups at 128, ends the iteration behind the trunk's launch:
      //  62.6 -> 46 us; 7.61-7.64 against 7.62-7.68 ms per step, 448: 7.64-7.67, 64: 7.68-7.71)
      if (f.ksplit != WgradKSplit::Level || k.level == 3 || F.total_wg >= 448 || (deterministic && F.total_wg >= 256)) break;
    }
    F.starts.push_back(F.total_wg);
    F.pair_off.assign(F.plans.size(), -1);
    if (deterministic) plan_pairs(F, cleared_target);
    for (const WgradDesc& d : ds) {
      F.flops += 2.0 * (double)d.N * d.OH * d.OW * d.Cout * d.Cin * f.T;
      F.abytes += 4.0 * ((double)d.N * ((double)d.Cin * d.Hin * d.Win + (double)d.Cout * d.OH * d.OW) + (double)d.Cout * d.Cin * f.T);
    }
    for (size_t i = 0, n = 0; i < descs.size(); ++i)
      if (L.desc_cat[i] == g) L.desc_S[i] = F.plans[n++].S;
  }
  return L;
}
