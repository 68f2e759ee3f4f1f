// Stand-alone check of the device LZW encoder's loop on the CPU.  lzw_encode_lanes (tiff_encode.hip) is __host__
// __device__; tiff_lzw_encode_twin runs it with one lane.  From a fixed seed this program encodes Gaussian int16 and float32 noise, a
// constant block, a half-constant block, a ramp and uniform random bytes -- each also after predictor 2 (horizontal differencing per
// row of 256 samples in the sample's width, wrapping) -- at lengths 0, 1, 2, 63, 64, 65, 255, 256, 257 and as whole 256 x 256 blocks, and
// demands for every case that the twin's bytes and size equal dbm_lzw_encode_tiles' and that dbm_lzw_decode returns the input; then, with
// capacities equal to, one below and far below the encoded size, that the twin returns 0 exactly where lzw_encode_one does and writes
// nothing outside its buffer.  Built with AddressSanitizer and UBSan on the host side, every buffer exactly as large as declared
// (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -x hip tools/lzw_encode_twin_check.cpp deepbedmap_amd/csrc/tiff_lzw.hip deepbedmap_amd/csrc/tiff_encode.hip \
//         -o lzw_encode_twin_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int dbm_lzw_encode_tiles(const void* tiles, size_t tile_bytes, int ntiles, void* out, size_t out_stride, size_t* out_sizes, int nthreads);
extern "C" int dbm_lzw_decode(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes);
size_t tiff_lzw_encode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}
static double gauss() {
  const double u = ((rnd() >> 11) + 1.0) / 9007199254740993.0, v = (rnd() >> 11) / 9007199254740992.0;
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

static long g_cases = 0, g_equal = 0, g_refused = 0;

static void fail(const char* what, size_t n, size_t cap, const char* why) {
  fprintf(stderr, "MISMATCH (%s): n %zu cap %zu: %s\n", what, n, cap, why);
  exit(1);
}

// both encoders on src[0, n) with `cap` bytes of room, each into a heap buffer of exactly cap bytes; returns the size (0: refused alike)
static size_t compare(const uint8_t* src, size_t n, size_t cap, const char* what) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);   // (an exact copy: a read at or past n is a heap overflow)
  if (n) memcpy(in, src, n);
  uint8_t* a = (uint8_t*)malloc(cap ? cap : 1);
  uint8_t* b = (uint8_t*)malloc(cap ? cap : 1);
  memset(a, 0xAA, cap ? cap : 1);
  memset(b, 0x55, cap ? cap : 1);
  size_t size_a = 0;
  const int rc = dbm_lzw_encode_tiles(in, n, 1, a, cap, &size_a, 1);
  const size_t size_b = tiff_lzw_encode_twin(in, n, b, cap);
  ++g_cases;
  if ((rc != 0) != (size_b == 0)) fail(what, n, cap, "one encoder refuses, the other does not");
  if (rc != 0) {
    ++g_refused;
    size_a = 0;
  } else {
    if (size_a != size_b) fail(what, n, cap, "sizes differ");
    if (memcmp(a, b, size_a) != 0) fail(what, n, cap, "bytes differ");
    uint8_t* back = (uint8_t*)malloc(n ? n : 1);
    size_t got = 0;
    if (dbm_lzw_decode(b, size_b, back, n, &got) != 0 || got != n || (n && memcmp(back, in, n) != 0)) fail(what, n, cap, "the stream does not decode to the input");
    free(back);
    ++g_equal;
  }
  free(in);
  free(a);
  free(b);
  return size_a;
}

static void check(const std::vector<uint8_t>& raw, const char* what) {
  const size_t n = raw.size();
  const size_t size = compare(raw.data(), n, n * 3 / 2 + 64, what);   // the slot of the device path
  if (size == 0) fail(what, n, n * 3 / 2 + 64, "refused with the full slot");
  const size_t caps[6] = {size, size - 1, size / 2, (size_t)2, (size_t)1, (size_t)0};
  for (size_t k = 0; k < 6; ++k) {
    const size_t got = compare(raw.data(), n, caps[k], what);
    if ((got != 0) != (caps[k] >= size)) fail(what, n, caps[k], "accepted or refused at the wrong capacity");
  }
}

// horizontal differencing per row of `row` samples of `w` bytes, wrapping; a trailing partial row is differenced as far as it goes
static std::vector<uint8_t> predictor2(const std::vector<uint8_t>& raw, size_t w, size_t row) {
  std::vector<uint8_t> out(raw);
  const size_t samples = raw.size() / w;
  for (size_t s = 0; s < samples; ++s) {
    if (s % row == 0) continue;
    uint32_t cur = 0, prev = 0;
    memcpy(&cur, raw.data() + s * w, w);
    memcpy(&prev, raw.data() + (s - 1) * w, w);
    const uint32_t d = cur - prev;
    memcpy(out.data() + s * w, &d, w);
  }
  return out;
}

int main() {
  const size_t whole = 256 * 256;
  std::vector<std::pair<std::string, std::pair<size_t, std::vector<uint8_t>>>> contents;   // name, (sample width, bytes of a 256 x 256 block)
  auto add = [&](const char* name, size_t w, const void* data) {
    std::vector<uint8_t> raw(whole * w);
    memcpy(raw.data(), data, raw.size());
    contents.push_back({name, {w, raw}});
  };
  {
    std::vector<int16_t> f(whole);
    for (auto& v : f) v = (int16_t)(300.0 * gauss());
    add("int16 noise", 2, f.data());
  }
  {
    std::vector<float> f(whole);
    for (auto& v : f) v = (float)(300.0 * gauss());
    add("float32 noise", 4, f.data());
  }
  {
    std::vector<int16_t> f(whole, (int16_t)-2000);
    add("constant", 2, f.data());
  }
  {
    std::vector<int16_t> f(whole, (int16_t)-2000);
    for (size_t i = whole / 2; i < whole; ++i) f[i] = (int16_t)(300.0 * gauss());
    add("half constant", 2, f.data());
  }
  {
    std::vector<int16_t> f(whole);
    for (size_t i = 0; i < whole; ++i) f[i] = (int16_t)(3 * (i % 256) + (i / 256));
    add("ramp", 2, f.data());
  }
  {
    std::vector<uint16_t> f(whole);
    for (auto& v : f) v = (uint16_t)rnd();
    add("uniform random bytes", 2, f.data());
  }
  const size_t lengths[9] = {0, 1, 2, 63, 64, 65, 255, 256, 257};
  for (auto& c : contents) {
    const size_t w = c.second.first;
    for (int pred = 1; pred <= 2; ++pred) {
      const std::vector<uint8_t> raw = pred == 2 ? predictor2(c.second.second, w, 256) : c.second.second;
      const std::string name = c.first + (pred == 2 ? " after predictor 2" : "");
      for (size_t len : lengths) check(std::vector<uint8_t>(raw.begin(), raw.begin() + (long)len), name.c_str());
      check(raw, name.c_str());
    }
  }
  printf("lzw_encode_twin_check: %ld cases, %ld encoded alike and decoded back, %ld refused alike, no mismatch\n", g_cases, g_equal, g_refused);
  return 0;
}
