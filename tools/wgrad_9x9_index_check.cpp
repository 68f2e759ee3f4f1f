// Stand-alone check on the CPU of the index arithmetic of wgrad_wave_dma_9x9_kernel.  The kernel takes its LDS layout, read
// offsets and validity table from deepbedmap_amd/csrc/wgrad_9x9_index.h; this program takes them from the same header and replays one
// workgroup's staging and K loop on a CPU array laid out as the LDS is.  No kernel runs and no HIP call is made.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I deepbedmap_amd/csrc tools/wgrad_9x9_index_check.cpp
//       -o wgrad_9x9_index_check && ./wgrad_9x9_index_check
//
// Per case (C_in, C_out of tests/test_gpu_wgrad_9x9_borders.py, N = 3), per workgroup (output tile, pair of input tiles):
//   - the planner (wgrad_plan.h) takes the wave-DMA form with 16-byte staging and asks for at least the LDS the layout needs;
//   - every 16-byte piece of the staging reads inside the tile's channels and lands inside its slab;
//   - every read of the K loop lies inside the launch's allocation and on a cell that was zeroed at kernel start or landed;
//   - the result equals a brute-force 3 x 3 weight gradient in 64-bit integers (integer-valued data: every fp32 sum is exact; every
//     cell of a tile is distinct, so a read that wraps into the neighbouring row or plane and is not multiplied by zero changes it);
//   - the result equals, bit for bit and element by element, a replay of the framed scheme the kernel had before (rows of 10 cells in
//     a frame of zeros, every one of the 369 MFMAs issued), which is the general kernel's arithmetic.
#include "wgrad_9x9_index.h"
#include "wgrad_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace wgrad9;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "wgrad_9x9_index_check: " __VA_ARGS__); fprintf(stderr, "  [%s, line %d]\n", #c, __LINE__); exit(1); } } while (0)

// the workgroup's LDS: `alloc` floats were requested, cells are uninitialised (0), zeroed at kernel start (1) or landed by DMA (2)
struct Lds {
  std::vector<float> v;
  std::vector<char> state;
  explicit Lds(size_t alloc) : v(alloc, 12345.f), state(alloc, 0) {}
  void zero_at_start(int floats) {
    CHECK((size_t)floats <= v.size(), "the kernel zeroes %d floats of %zu", floats, v.size());
    for (int e = 0; e < floats; ++e) v[e] = 0.f, state[e] = 1;
  }
  void land16(int dst, const float* src) {  // one lane of a 16-byte LDS-DMA instruction
    CHECK(dst >= 0 && dst % 4 == 0 && (size_t)dst + 4 <= v.size(), "DMA destination %d", dst);
    for (int k = 0; k < 4; ++k) v[dst + k] = src[k], state[dst + k] = 2;
  }
  float rd(int i, const char* what, int s, int t, int j, int kh) const {
    CHECK(i >= 0 && (size_t)i < v.size(), "%s read at %d leaves the allocation (step %d tap %d lane %d,%d)", what, i, s, t, j, kh);
    CHECK(state[i] != 0, "%s read at %d is on an uninitialised cell (step %d tap %d lane %d,%d)", what, i, s, t, j, kh);
    return v[i];
  }
};

typedef std::vector<float> Acc;  // [wave][t][o][c], 2 * 9 * 32 * 32: the accumulators of a workgroup's two wavefronts
static float& at(Acc& a, int wave, int t, int o, int c) { return a[((wave * T + t) * 32 + o) * 32 + c]; }

// v_mfma_f32_32x32x2_f32: D[o][c] += A[o][0] B[c][0] + A[o][1] B[c][1], lane (j, kh) holds A[j][kh] and B[j][kh]
static void mfma(Acc& acc, int wave, int t, const float (&a)[32][2], const float (&b)[32][2]) {
  for (int o = 0; o < 32; ++o)
    for (int c = 0; c < 32; ++c) {
      float& d = at(acc, wave, t, o, c);
      d += a[o][0] * b[c][0];
      d += a[o][1] * b[c][1];
    }
}

struct Case {
  int N, Cin, Cout;
  std::vector<float> x, dy;  // (N, Cin, 81), (N, Cout, 81)
};

// one workgroup of the kernel as it is: output tile by, input tiles 2 g and 2 g + 1
static Acc replay_slab(const Case& k, int by, int g, size_t alloc_floats, long* mfmas) {
  Acc acc(2 * T * 32 * 32, 0.f);
  Lds lds(alloc_floats);
  lds.zero_at_start(LDS_FLOATS);
  const int cout0 = 32 * by, nco = std::min(32, k.Cout - cout0);
  for (int n = 0; n < k.N; ++n) {
    const float* srcy = &k.dy[((size_t)n * k.Cout + cout0) * PLANE];
    CHECK(nco * PLANE % 4 == 0, "dy run of %d floats", nco * PLANE);
    for (int i = 0; i < nco * PLANE / 4; ++i) {
      CHECK(4 * i + 4 <= SLAB, "dy piece %d leaves the slab", i);
      lds.land16(LDS_Y + 4 * i, srcy + 4 * i);
    }
    for (int wave = 0; wave < 2; ++wave) {
      const int cin_w = 32 * (2 * g + wave), nci = std::max(0, std::min(32, k.Cin - cin_w));
      CHECK(nci * PLANE % 4 == 0, "x run of %d floats", nci * PLANE);
      for (int i = 0; i < nci * PLANE / 4; ++i) {
        CHECK(4 * i + 4 <= SLAB, "x piece %d leaves the slab", i);
        CHECK((size_t)(cin_w * PLANE + 4 * i + 4) <= (size_t)k.Cin * PLANE, "x piece %d leaves the image", i);
        lds.land16(lds_x(wave) + 4 * i, &k.x[((size_t)n * k.Cin + cin_w) * PLANE + 4 * i]);
      }
    }
    for (int wave = 0; wave < 2; ++wave) {
      if (32 * (2 * g + wave) >= k.Cin) continue;  // wave_active
      for (int s = 0; s < STEPS; ++s)
        for (int t = 0; t < T; ++t) {
          const int v = valid(s, t);
          if (v == NONE) continue;
          CHECK(step_uses(s, v), "step %d tap %d", s, t);
          float a[32][2], b[32][2];
          for (int j = 0; j < 32; ++j)
            for (int kh = 0; kh < 2; ++kh) {
              a[j][kh] = lds.rd(a_base(v, j, kh) + a_off(s), "A", s, t, j, kh);
              b[j][kh] = lds.rd(b_base(wave, j, kh) + b_off(s, t), "B", s, t, j, kh);
              // a half outside the plane takes its A value from the zero region, which nothing writes after kernel start
              if (!tap_inside(2 * s + kh, t)) {
                const int ai = a_base(v, j, kh) + a_off(s);
                CHECK(ai >= LDS_ZERO && ai < LDS_ZERO + ZERO_FLOATS && lds.state[ai] == 1, "A of an outside half at %d (step %d tap %d)", ai, s, t);
              }
            }
          mfma(acc, wave, t, a, b);
          ++*mfmas;
        }
    }
  }
  return acc;
}

// the same workgroup with the framed x planes: dy slab, 4 zeros, 2 x 32 planes of (9 + 2) rows of (9 + 1) cells; position q has dy offset q
// and x offset q + q / 9; the kh = 1 lanes are one cell further, two where 2 s is a row's last position; the padding position reads A from
// the zero guard behind the slab and B from position 0's cells
static Acc replay_framed(const Case& k, int by, int g) {
  constexpr int W1 = W + 1, PS = (H + 2) * W1;
  Acc acc(2 * T * 32 * 32, 0.f);
  std::vector<float> lds(SLAB + 4 + 2 * 32 * PS, 0.f);
  const int cout0 = 32 * by, nco = std::min(32, k.Cout - cout0);
  for (int n = 0; n < k.N; ++n) {
    memcpy(&lds[0], &k.dy[((size_t)n * k.Cout + cout0) * PLANE], sizeof(float) * nco * PLANE);
    for (int wave = 0; wave < 2; ++wave) {
      const int cin_w = 32 * (2 * g + wave), nci = std::max(0, std::min(32, k.Cin - cin_w));
      float* X = &lds[SLAB + 4 + wave * 32 * PS];
      for (int c = 0; c < nci; ++c)
        for (int q = 0; q < PLANE; ++q) X[c * PS + (q / W + 1) * W1 + q % W] = k.x[((size_t)n * k.Cin + cin_w + c) * PLANE + q];
      if (nci == 0) continue;
      for (int s = 0; s < STEPS; ++s)
        for (int t = 0; t < T; ++t) {
          float a[32][2], b[32][2];
          const int kp = 2 * s, xo = kp + kp / W;
          const bool last = s == STEPS - 1;
          for (int j = 0; j < 32; ++j)
            for (int kh = 0; kh < 2; ++kh) {
              const int xrow = SLAB + 4 + wave * 32 * PS - 1 + j * PS;
              const int ap = last ? (kh ? SLAB - (PLANE - 1) : j * PLANE) : j * PLANE + kh;
              const int bp = last ? (kh ? xrow - (PLANE - 1 + (PLANE - 1) / W) : xrow) : (kp % W == W - 1 ? xrow + 2 * kh : xrow + kh);
              a[j][kh] = lds.at(ap + kp);
              b[j][kh] = lds.at(bp + xo + (t / 3) * W1 + t % 3);
            }
          mfma(acc, wave, t, a, b);
        }
    }
  }
  return acc;
}

int main() {
  static_assert(band_mfmas() == 339, "MFMAs per band");
  const int shapes[][2] = {{32, 32}, {64, 32}, {96, 32}, {160, 32}, {192, 64}, {64, 16}, {36, 32}};
  long checked = 0;
  for (const auto& sh : shapes) {
    Case k;
    k.N = 3, k.Cin = sh[0], k.Cout = sh[1];
    k.x.resize((size_t)k.N * k.Cin * PLANE);
    k.dy.resize((size_t)k.N * k.Cout * PLANE);
    // every cell of a 32-channel tile is distinct (and differs between images); dy in -2 .. 2
    for (int n = 0; n < k.N; ++n) {
      for (int c = 0; c < k.Cin; ++c)
        for (int q = 0; q < PLANE; ++q) k.x[((size_t)n * k.Cin + c) * PLANE + q] = (float)((c % 32) * PLANE + q + 1 + 3000 * n) * ((c + q) % 2 ? -1.f : 1.f);
      for (int o = 0; o < k.Cout; ++o)
        for (int q = 0; q < PLANE; ++q) k.dy[((size_t)n * k.Cout + o) * PLANE + q] = (float)((o * 5 + q * 3 + n) % 5 - 2);
    }
    // what the launch allocates for this layer
    alignas(16) static float fake[4];
    WgradDesc d;
    memset(&d, 0, sizeof(d));
    d.x = fake, d.dy = fake;
    d.xsn = (long)k.Cin * PLANE, d.xsc = PLANE, d.Cin = k.Cin, d.Hin = H, d.Win = W;
    d.dysn = (long)k.Cout * PLANE, d.dysc = PLANE, d.Cout = k.Cout, d.OH = H, d.OW = W;
    d.KH = d.KW = 3, d.stride = 1, d.pad = 1, d.N = k.N, d.scale = 1.f;
    WgradPlan p;
    memset(&p, 0, sizeof(p));
    const size_t bytes = plan_wave_dma(d, p, WgradSplit());
    CHECK(bytes != 0 && p.fast && p.IB == 1, "C_in %d C_out %d: not the wave-DMA form with 16-byte staging", k.Cin, k.Cout);
    CHECK(bytes >= sizeof(float) * LDS_FLOATS, "the plan asks for %zu bytes, the layout needs %zu", bytes, sizeof(float) * LDS_FLOATS);
    CHECK(p.groups == (k.Cin + 63) / 64 && p.coutTiles == (k.Cout + 31) / 32, "groups %d coutTiles %d", p.groups, p.coutTiles);
    for (int by = 0; by < p.coutTiles; ++by)
      for (int g = 0; g < p.groups; ++g) {
        long mfmas = 0;
        Acc got = replay_slab(k, by, g, bytes / sizeof(float), &mfmas);
        const int waves = 32 * (2 * g + 1) < k.Cin ? 2 : 1;
        CHECK(mfmas == (long)waves * k.N * band_mfmas(), "%ld MFMAs", mfmas);
        Acc framed = replay_framed(k, by, g);
        for (size_t i = 0; i < got.size(); ++i)
          CHECK(memcmp(&got[i], &framed[i], sizeof(float)) == 0, "C_in %d C_out %d tile %d group %d element %zu: %.9g, framed scheme %.9g", k.Cin,
                k.Cout, by, g, i, got[i], framed[i]);
        for (int wave = 0; wave < 2; ++wave)
          for (int t = 0; t < T; ++t)
            for (int o = 0; o < 32; ++o)
              for (int c = 0; c < 32; ++c) {
                const int oo = 32 * by + o, cc = 32 * (2 * g + wave) + c;
                int64_t ref = 0, mass = 0;
                if (oo < k.Cout && cc < k.Cin)
                  for (int n = 0; n < k.N; ++n)
                    for (int q = 0; q < PLANE; ++q) {
                      const int r = q / W + t / 3 - 1, cl = q % W + t % 3 - 1;
                      if (r < 0 || r >= H || cl < 0 || cl >= W) continue;
                      const int64_t term = (int64_t)k.dy[((size_t)n * k.Cout + oo) * PLANE + q] * (int64_t)k.x[((size_t)n * k.Cin + cc) * PLANE + r * W + cl];
                      ref += term, mass += term < 0 ? -term : term;
                    }
                CHECK(mass < (1 << 24), "the sums of this case are not exact in fp32 (%lld)", (long long)mass);
                CHECK((double)at(got, wave, t, o, c) == (double)ref, "C_in %d C_out %d gW[%d][%d][%d]: %.9g, brute force %lld", k.Cin, k.Cout, oo, cc, t,
                      at(got, wave, t, o, c), (long long)ref);
                ++checked;
              }
      }
  }
  printf("wgrad_9x9_index_check: ok (%ld elements, %d MFMAs per band, %d of %d LDS floats)\n", checked, band_mfmas(), LDS_FLOATS,
         SLAB + 4 + 64 * 110 + 82 + 8);
  return 0;
}
