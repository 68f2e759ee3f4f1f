// Stand-alone robustness check of the device LZW decoder's loop on the CPU.  lzw_decode_lanes (tiff_decode.hip) is
// __host__ __device__; tiff_lzw_decode_twin runs it with one lane.  This program feeds it, from a fixed seed, valid streams (noise,
// constant, half constant, ramps -- the contents of tests/test_gpu_geotiff_read.py -- encoded by dbm_lzw_encode_tiles, plus any stream
// files named on the command line), a few thousand mutations of each (truncations, byte flips, edits at the byte offsets where the code
// width changes, second code forced to 4095) and all-zero / all-ones inputs, with output capacities equal to, above and below the
// decoded size, and demands that it agrees with the host decoder (dbm_lzw_decode) on success / failure, size and bytes.  Built with
// AddressSanitizer and UBSan on the host side, every buffer exactly as large as declared (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -x hip tools/lzw_twin_check.cpp deepbedmap_amd/csrc/tiff_lzw.hip deepbedmap_amd/csrc/tiff_decode.hip -o lzw_twin_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int dbm_lzw_encode_tiles(const void* tiles, size_t tile_bytes, int ntiles, void* out, size_t out_stride, size_t* out_sizes, int nthreads);
extern "C" int dbm_lzw_decode(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes);
size_t tiff_lzw_decode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}
static double gauss() {
  const double u = ((rnd() >> 11) + 1.0) / 9007199254740993.0, v = (rnd() >> 11) / 9007199254740992.0;
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

static long g_cases = 0, g_ok = 0, g_rejected = 0;

// one comparison: both decoders on src[0, n) with `cap` bytes of output, each into a heap buffer of exactly cap bytes
static void compare(const uint8_t* src, size_t n, size_t cap, const char* what) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);   // (an exact copy: a read past n is a heap overflow)
  if (n) memcpy(in, src, n);
  uint8_t* a = (uint8_t*)malloc(cap ? cap : 1);
  uint8_t* b = (uint8_t*)malloc(cap ? cap : 1);
  memset(a, 0xAA, cap ? cap : 1);
  memset(b, 0x55, cap ? cap : 1);
  size_t got_a = 0;
  const int rc = dbm_lzw_decode(in, n, a, cap, &got_a);
  const size_t got_b = tiff_lzw_decode_twin(in, n, b, cap);
  ++g_cases;
  const bool fail_a = rc != 0, fail_b = got_b == (size_t)-1;
  if (fail_a != fail_b || (!fail_a && (got_a != got_b || memcmp(a, b, got_a) != 0))) {
    fprintf(stderr, "MISMATCH (%s): n %zu cap %zu host rc %d size %zu, twin size %zd\n", what, n, cap, rc, got_a, (ssize_t)got_b);
    exit(1);
  }
  if (fail_a) ++g_rejected; else ++g_ok;
  free(in);
  free(a);
  free(b);
}

static void torture(const std::vector<uint8_t>& stream, size_t decoded, int mutations, const char* what) {
  const size_t n = stream.size();
  const size_t caps[4] = {decoded, decoded + 16, decoded / 2, decoded ? decoded - 1 : 0};
  for (size_t cap : caps) compare(stream.data(), n, cap, what);
  // the byte offsets at which the code width changes (9 -> 10 -> 11 -> 12 bits) and the table starts over, for an incompressible start
  const size_t edges[5] = {2, 285, 925, 2333, 5403};
  std::vector<uint8_t> m;
  for (int k = 0; k < mutations; ++k) {
    m = stream;
    const int kind = (int)(rnd() % 5);
    size_t len = n;
    if (kind == 0) {
      len = (size_t)(rnd() % (n + 1));                                   // truncation
    } else if (kind == 1) {
      m[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));                     // one bit
    } else if (kind == 2) {
      m[rnd() % n] = (uint8_t)rnd();                                     // one byte
    } else if (kind == 3) {
      const size_t at = edges[rnd() % 5] + (size_t)(rnd() % 5);          // around a width boundary
      if (at < n) m[at >= 2 ? at - 2 : at] ^= (uint8_t)(rnd() | 1);
    } else {
      const size_t at = (size_t)(rnd() % n);                              // a run of ones: codes 4095 / beyond `next`
      for (size_t i = at; i < n && i < at + 1 + rnd() % 3; ++i) m[i] = 0xFF;
    }
    compare(m.data(), len, caps[rnd() % 4], what);
  }
  // the second code replaced by 4095 (as far as 9 bits reach: 511), and the stream cut at half its length
  m = stream;
  if (n > 3) { m[1] |= 0x7F; m[2] |= 0xC0; compare(m.data(), n, decoded, what); }
  compare(stream.data(), n / 2, decoded, what);
}

static std::vector<uint8_t> encode(const std::vector<uint8_t>& raw) {
  std::vector<uint8_t> out(raw.size() * 3 / 2 + 64);
  size_t size = 0;
  if (dbm_lzw_encode_tiles(raw.data(), raw.size(), 1, out.data(), out.size(), &size, 1) != 0) { fprintf(stderr, "encode failed\n"); exit(1); }
  out.resize(size);
  return out;
}

int main(int argc, char** argv) {
  const int mutations = 1500;
  std::vector<std::pair<std::string, std::vector<uint8_t>>> contents;
  {  // float32 Gaussian noise, a strip of 16 x 300 samples
    std::vector<float> f(16 * 300);
    for (auto& v : f) v = (float)(1000.0 * gauss());
    std::vector<uint8_t> raw(f.size() * 4);
    memcpy(raw.data(), f.data(), raw.size());
    contents.push_back({"float32 noise", raw});
  }
  {  // int16 noise
    std::vector<int16_t> f(16 * 300);
    for (auto& v : f) v = (int16_t)(300.0 * gauss());
    std::vector<uint8_t> raw(f.size() * 2);
    memcpy(raw.data(), f.data(), raw.size());
    contents.push_back({"int16 noise", raw});
  }
  {  // a constant 256 x 256 int16 tile: KwKwK at every step, strings of several hundred bytes
    std::vector<int16_t> f(256 * 256, (int16_t)-2000);
    std::vector<uint8_t> raw(f.size() * 2);
    memcpy(raw.data(), f.data(), raw.size());
    contents.push_back({"constant tile", raw});
  }
  {  // half constant, half noise
    std::vector<int16_t> f(256 * 256, (int16_t)-2000);
    for (size_t i = f.size() / 2; i < f.size(); ++i) f[i] = (int16_t)(300.0 * gauss());
    std::vector<uint8_t> raw(f.size() * 2);
    memcpy(raw.data(), f.data(), raw.size());
    contents.push_back({"half constant", raw});
  }
  {  // differenced smooth terrain (what predictor 2 leaves): few distinct bytes
    std::vector<uint8_t> raw(40000);
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)((i / 7) % 3);
    contents.push_back({"ramp", raw});
  }
  contents.push_back({"one byte", std::vector<uint8_t>(1, 7)});
  for (auto& c : contents) {
    const std::vector<uint8_t> s = encode(c.second);
    // the valid stream decodes to the content in both
    std::vector<uint8_t> back(c.second.size() + 1);
    if (tiff_lzw_decode_twin(s.data(), s.size(), back.data(), c.second.size()) != c.second.size() ||
        memcmp(back.data(), c.second.data(), c.second.size()) != 0) {
      fprintf(stderr, "twin does not decode '%s'\n", c.first.c_str());
      return 1;
    }
    torture(s, c.second.size(), s.size() > 0 ? mutations : 0, c.first.c_str());
  }
  // stream files: "<decoded size>:<path>"
  for (int i = 1; i < argc; ++i) {
    const char* colon = strchr(argv[i], ':');
    if (!colon) { fprintf(stderr, "argument %d: expected <decoded size>:<path>\n", i); return 2; }
    const size_t decoded = (size_t)atol(argv[i]);
    FILE* f = fopen(colon + 1, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", colon + 1); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.insert(s.end(), buf, buf + got);
    fclose(f);
    std::vector<uint8_t> back(decoded + 1);
    if (tiff_lzw_decode_twin(s.data(), s.size(), back.data(), decoded) != decoded) { fprintf(stderr, "twin does not decode %s\n", colon + 1); return 1; }
    torture(s, decoded, mutations, colon + 1);
  }
  // all-zero and all-ones inputs
  for (size_t n : {0, 1, 2, 3, 9, 64, 1000, 20000}) {
    std::vector<uint8_t> z(n, 0x00), o(n, 0xFF);
    for (size_t cap : {0, 1, 100, 70000}) {
      compare(z.data(), n, cap, "zeros");
      compare(o.data(), n, cap, "ones");
    }
  }
  printf("lzw_twin_check: %ld cases, %ld decoded alike, %ld rejected alike, no mismatch\n", g_cases, g_ok, g_rejected);
  return 0;
}
