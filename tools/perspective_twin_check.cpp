// Stand-alone check of the perspective view on the CPU.  dbm_grid_perspective_host runs the kernel's own cell, wall and
// colour functions under the plain walk; perspective_render_host(..., skipping = true) runs the DEVICE's traversal -- strips of 64, 8 and
// 1 cells, blocks skipped by their maxima, the early stop -- on host threads.  From a fixed seed this program makes DEM-like planes of
// 37 x 29 (with a NaN patch, NaN nodes on the boundary and a +inf and a -inf node), 150 x 210 and 9 x 130, renders each from six views
// (the reference's, two along grid axes, one along the cells' diagonals, the two limits of the elevation) with and without a facade,
// at a level below and above the samples, and requires that both traversals give the same bytes and the same ids, that some surface is
// seen, and that the refusals are refusals.  Built with AddressSanitizer and UBSan on the host side (tools/README.md), so every index
// the traversal makes into the plane, the drape and the block maxima is checked:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -I include -x hip tools/perspective_twin_check.cpp deepbedmap_amd/csrc/perspective.hip \
//         -o perspective_twin_check
// Never run on a GPU machine and not part of the pytest suite: it needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels.h"

extern "C" int dbm_grid_perspective_host(const float* plane, long H, long W, const uint8_t* drape, int drape_channels, const double* view, long Wo,
                                         long Ho, const uint8_t* facade_rgba, const uint8_t* background_rgba, uint8_t* out, int32_t* hits,
                                         int nthreads);
// (api.hip is not linked: the message of a refusal goes to stderr)
void api_record_error(dbm_ctx*, const char* what) { std::fprintf(stderr, "refused: %s\n", what); }

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

static int failures = 0, cases = 0;

static std::vector<float> plane_of(long H, long W) {
  std::vector<float> z((size_t)(H * W));
  for (long r = 0; r < H; ++r)
    for (long c = 0; c < W; ++c) {
      double v = 1400.0 * std::sin(0.11 * r + 0.3) * std::cos(0.07 * c - 0.2) + 700.0 * std::sin(0.031 * (r + 2.0 * c)) + 600.0 * (rnd() - 0.5);
      z[(size_t)(r * W + c)] = (float)(v < -2500.0 ? -2500.0 : (v > 2500.0 ? 2500.0 : v));
    }
  if (H == 37 && W == 29) {
    for (long r = 10; r < 15; ++r)
      for (long c = 8; c < 12; ++c) z[(size_t)(r * W + c)] = NAN;
    z[20] = NAN;
    z[(size_t)(36 * W + 3)] = NAN;
    z[(size_t)(22 * W + 17)] = INFINITY;
    z[(size_t)(30 * W + 9)] = -INFINITY;
  }
  return z;
}

static void check(long H, long W, double azimuth, double elevation, double level, bool facade_on, int channels, long width) {
  ++cases;
  const std::vector<float> z = plane_of(H, W);
  std::vector<uint8_t> drape((size_t)(H * W * channels));
  for (auto& b : drape) b = (uint8_t)(256.0 * rnd());
  const double pi = 3.14159265358979323846, zfac = 10.0 / 250.0;
  double sin_a = std::sin(azimuth * pi / 180.0), cos_a = std::cos(azimuth * pi / 180.0);
  if (azimuth == 0.0) { sin_a = 0.0; cos_a = 1.0; }
  if (azimuth == 90.0) { sin_a = 1.0; cos_a = 0.0; }
  const double e = elevation * pi / 180.0, sin_e = std::sin(e), cos_e = std::cos(e), tan_e = std::tan(e);
  double zmin = INFINITY, zmax = -INFINITY;
  for (float v : z)
    if (std::isfinite(v)) { zmin = v < zmin ? v : zmin; zmax = v > zmax ? v : zmax; }
  const double h_lo = std::fmin(0.0, (zmin - level) * zfac), h_hi = std::fmax(0.0, (zmax - level) * zfac);
  double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  for (double east : {0.0, (double)(W - 1)})
    for (double north : {0.0, -(double)(H - 1)})
      for (double height : {h_lo, h_hi}) {
        const double x = -east * cos_a + north * sin_a, y = (-east * sin_a - north * cos_a) * sin_e + height * cos_e;
        xmin = std::fmin(xmin, x); xmax = std::fmax(xmax, x); ymin = std::fmin(ymin, y); ymax = std::fmax(ymax, y);
      }
  const double step = (xmax - xmin) / (double)width;
  const long Wo = width, Ho = (long)std::ceil((ymax - ymin) / step);
  const double view[9] = {sin_a, cos_a, sin_e, tan_e, level, zfac, xmin, ymax, step};
  const uint8_t facade[4] = {128, 128, 128, 255}, background[4] = {1, 2, 3, 0};
  std::vector<uint8_t> plain((size_t)(Wo * Ho * 4)), skipped((size_t)(Wo * Ho * 4));
  std::vector<int32_t> plain_ids((size_t)(Wo * Ho)), skipped_ids((size_t)(Wo * Ho));
  if (dbm_grid_perspective_host(z.data(), H, W, drape.data(), channels, view, Wo, Ho, facade_on ? facade : nullptr, background, plain.data(),
                                plain_ids.data(), 3) != 0) {
    std::fprintf(stderr, "%ldx%ld A %g E %g: refused\n", H, W, azimuth, elevation);
    ++failures;
    return;
  }
  PerspLaunch a{};
  a.plane = z.data(); a.H = H; a.W = W;
  a.drape = drape.data(); a.channels = channels;
  a.v = PerspView{sin_a, cos_a, sin_e, tan_e, level, zfac, xmin, ymax, step};
  a.Wo = Wo; a.Ho = Ho;
  a.facade_on = facade_on;
  std::memcpy(a.facade, facade, 4);
  std::memcpy(a.background, background, 4);
  a.out = skipped.data(); a.hits = skipped_ids.data();
  perspective_render_host(a, true, 3);
  long seen = 0, walls = 0, other = 0;
  for (size_t p = 0; p < plain_ids.size(); ++p) {
    seen += plain_ids[p] >= 0;
    walls += plain_ids[p] == -2;
    other += plain_ids[p] != skipped_ids[p];
  }
  other += std::memcmp(plain.data(), skipped.data(), plain.size()) != 0;
  std::printf("%3ldx%-3ld A %5.1f E %2.0f level %6.0f %s %d ch: %ld x %ld, %ld surface, %ld wall pixels, %ld differ\n", H, W, azimuth, elevation, level,
              facade_on ? "walls" : "open ", channels, Wo, Ho, seen, walls, other);
  if (other != 0 || seen == 0 || (!facade_on && walls != 0)) ++failures;
}

static void refusals() {
  ++cases;
  const std::vector<float> z = plane_of(5, 5);
  std::vector<uint8_t> drape(75), out(64);
  const uint8_t rgba[4] = {0, 0, 0, 0};
  double view[9] = {0.6, 0.8, 0.5, 0.57, -1400.0, 0.04, -3.0, 3.0, 1.0};
  int bad = 0;
  bad += dbm_grid_perspective_host(z.data(), 5, 5, drape.data(), 3, view, 4, 4, nullptr, rgba, out.data(), nullptr, 1) != 0;
  bad += dbm_grid_perspective_host(nullptr, 5, 5, drape.data(), 3, view, 4, 4, nullptr, rgba, out.data(), nullptr, 1) != 1;
  bad += dbm_grid_perspective_host(z.data(), 5, 5, drape.data(), 2, view, 4, 4, nullptr, rgba, out.data(), nullptr, 1) != 1;
  bad += dbm_grid_perspective_host(z.data(), 5, 5, drape.data(), 3, view, 4, 0, nullptr, rgba, out.data(), nullptr, 1) != 1;
  view[8] = 0.0;
  bad += dbm_grid_perspective_host(z.data(), 5, 5, drape.data(), 3, view, 4, 4, nullptr, rgba, out.data(), nullptr, 1) != 1;
  view[8] = NAN;
  bad += dbm_grid_perspective_host(z.data(), 5, 5, drape.data(), 3, view, 4, 4, nullptr, rgba, out.data(), nullptr, 1) != 1;
  if (bad) {
    std::fprintf(stderr, "refusals: %d wrong statuses\n", bad);
    ++failures;
  }
}

int main() {
  const double views[6][2] = {{202.5, 60.0}, {0.0, 60.0}, {90.0, 30.0}, {45.0, 35.0}, {315.0, 1.0}, {135.0, 89.0}};
  const long shapes[3][3] = {{37, 29, 96}, {150, 210, 200}, {9, 130, 160}};
  for (const auto& s : shapes)
    for (const auto& v : views)
      for (int setting = 0; setting < 4; ++setting)
        check(s[0], s[1], v[0], v[1], setting & 1 ? 2600.0 : -1400.0, (setting & 2) == 0, setting & 1 ? 3 : 4, s[2]);
  refusals();
  std::printf("perspective_twin_check: %d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
