// Stand-alone check of the PNG band encoder on the CPU.  dbm_png_encode_host runs the device's own texts with one lane:
// png_band_byte (png_encode.hip) and deflate_encode_lanes with framing 1 / 2 (deflate_encode.hip).  From a fixed seed this program makes
// smooth, constant and uniform random images of 1 x 1, 3 x 5 x 3, 37 x 29 x 4, 40 x 33 x 1 and 96 x 200 x 4, encodes each with filters
// 0, 1, 2 and band_rows 1, 5 and H on 1 and 3 threads into buffers exactly as large as the entry point demands, and requires that
// every segment stays within n + n / 8 + 16 bytes, that 78 01 + the segments + the Adler-32 joined from the segments' sums is a zlib
// stream whose `uncompress` returns the filtered scanlines computed here by a separate loop, and that a range of bands gives the
// bytes of those bands.  Built with AddressSanitizer and UBSan on the host side (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -I include -x hip tools/png_twin_check.cpp deepbedmap_amd/csrc/png_encode.hip \
//         deepbedmap_amd/csrc/deflate_encode.hip -lz -o png_twin_check
// Never run on a GPU machine and not part of the pytest suite: it needs no device.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct dbm_ctx;
extern "C" int dbm_png_encode_host(const void* image, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                                   void* out, size_t out_capacity, size_t* sizes, uint32_t* adlers, int nthreads);
// (api.hip is not linked: the message of a refusal goes to stderr)
void api_record_error(dbm_ctx*, const char* what) { std::fprintf(stderr, "refused: %s\n", what); }

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}

static uint32_t combine(uint32_t a1, uint32_t a2, size_t len2) {
  const uint64_t M = 65521, s1 = a1 & 0xFFFF, s2 = a1 >> 16, t1 = a2 & 0xFFFF, t2 = a2 >> 16;
  const uint64_t a = (s1 + t1 + M - 1) % M, b = (s2 + t2 + (len2 % M) * ((s1 + M - 1) % M)) % M;
  return (uint32_t)((b << 16) | a);
}

static int failures = 0, cases = 0;
#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, " (%s)\n", #cond); ++failures; return; } } while (0)

static void check(const std::vector<uint8_t>& image, long H, long W, int ch, int filter, int band_rows, int threads) {
  ++cases;
  const long row = W * ch;
  std::vector<uint8_t> lines((size_t)H * (row + 1));
  for (long r = 0; r < H; ++r) {
    lines[r * (row + 1)] = (uint8_t)filter;
    for (long x = 0; x < row; ++x) {
      int prior = 0;
      if (filter == 1 && x >= ch) prior = image[r * row + x - ch];
      if (filter == 2 && r > 0) prior = image[(r - 1) * row + x];
      lines[r * (row + 1) + 1 + x] = (uint8_t)(image[r * row + x] - prior);
    }
  }
  const long rows = band_rows < H ? band_rows : H, bands = (H + band_rows - 1) / band_rows;
  const size_t n = (size_t)rows * (row + 1), slot = n + n / 8 + 16, worst = (slot + 1) & ~(size_t)1;
  std::vector<uint8_t> out((size_t)bands * worst);
  std::vector<size_t> sizes(bands);
  std::vector<uint32_t> adlers(bands);
  REQUIRE(dbm_png_encode_host(image.data(), H, W, ch, filter, band_rows, 0, (int)bands, out.data(), out.size(), sizes.data(), adlers.data(), threads) == 0,
          "%ldx%ldx%d filter %d rows %d: refused", H, W, ch, filter, band_rows);
  std::vector<uint8_t> stream{0x78, 0x01};
  uint32_t adler = 1;
  size_t at = 0;
  for (long b = 0; b < bands; ++b) {
    const size_t len = (size_t)((b == bands - 1 ? H - b * band_rows : band_rows)) * (row + 1);
    REQUIRE(sizes[b] > 0 && sizes[b] <= len + len / 8 + 16, "band %ld: %zu bytes for %zu", b, sizes[b], len);
    REQUIRE(adlers[b] == (uint32_t)adler32(adler32(0, nullptr, 0), lines.data() + (size_t)b * n, (uInt)len), "band %ld: Adler-32", b);
    stream.insert(stream.end(), out.begin() + at, out.begin() + at + sizes[b]);
    adler = combine(adler, adlers[b], len);
    at += (sizes[b] + 1) & ~(size_t)1;
  }
  for (int k = 3; k >= 0; --k) stream.push_back((uint8_t)(adler >> (8 * k)));
  std::vector<uint8_t> back(lines.size() + 1);
  uLongf got = (uLongf)back.size();
  REQUIRE(uncompress(back.data(), &got, stream.data(), (uLong)stream.size()) == Z_OK, "%ldx%ldx%d filter %d rows %d: zlib refuses the stream", H, W,
          ch, filter, band_rows);
  REQUIRE(got == lines.size() && std::memcmp(back.data(), lines.data(), lines.size()) == 0, "%ldx%ldx%d filter %d rows %d: other bytes", H, W, ch,
          filter, band_rows);
  if (bands >= 3) {   // bands 1 .. bands - 2 alone: exactly their bytes
    std::vector<uint8_t> part((size_t)(bands - 2) * worst);
    std::vector<size_t> psizes(bands - 2);
    std::vector<uint32_t> padlers(bands - 2);
    REQUIRE(dbm_png_encode_host(image.data(), H, W, ch, filter, band_rows, 1, (int)bands - 2, part.data(), part.size(), psizes.data(), padlers.data(), 1) == 0,
            "range refused");
    size_t skip = (sizes[0] + 1) & ~(size_t)1, total = 0;
    for (long b = 0; b < bands - 2; ++b) {
      REQUIRE(psizes[b] == sizes[b + 1] && padlers[b] == adlers[b + 1], "range: band %ld differs", b + 1);
      total += (psizes[b] + 1) & ~(size_t)1;
    }
    REQUIRE(std::memcmp(part.data(), out.data() + skip, total) == 0, "range: other bytes");
  }
}

int main() {
  const long shapes[5][3] = {{1, 1, 4}, {3, 5, 3}, {37, 29, 4}, {40, 33, 1}, {96, 200, 4}};
  for (const auto& s : shapes) {
    const long H = s[0], W = s[1];
    const int ch = (int)s[2];
    for (int content = 0; content < 3; ++content) {
      std::vector<uint8_t> image((size_t)H * W * ch);
      for (long r = 0; r < H; ++r)
        for (long c = 0; c < W; ++c)
          for (int k = 0; k < ch; ++k)
            image[(r * W + c) * ch + k] = content == 0 ? (uint8_t)((3 * r + 5 * c + 40 * k) % 251) : content == 1 ? (uint8_t)200 : (uint8_t)rnd();
      for (int filter = 0; filter < 3; ++filter)
        for (int band_rows : {1, 5, (int)H})
          for (int threads : {1, 3}) check(image, H, W, ch, filter, band_rows, threads);
    }
  }
  std::printf("png_twin_check: %d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
