// Stand-alone robustness check of the device inflate decoder's loop on the CPU.  inflate_lanes (tiff_inflate.hip) is
// __host__ __device__; tiff_inflate_twin runs it with one lane.  This program feeds it, from a fixed seed, valid zlib streams (float32
// noise, row-differenced int16 noise, a constant tile, zeros, half constant, a ramp, skewed symbols, one byte, nothing -- the kinds of
// content in tests/test_gpu_geotiff_inflate.py -- compressed by zlib with every deflateInit2 strategy, levels 0 / 1 / 6 / 9, window bits 9 and a
// Z_FULL_FLUSH in the middle, plus any stream files named on the command line: tests/inflate_restatement.py writes the streams zlib
// never emits), a few thousand mutations of each (truncations, bit and byte flips, edits inside the first block's header, runs of ones
// that force extra bits high, trailer flips) and all-zero / all-ones inputs, with output capacities equal to, above and below the
// decoded size, and demands that it agrees with zlib's `uncompress` on success / failure, and on success in size and bytes.  Built with
// AddressSanitizer and UBSan on the host side, every buffer exactly as large as declared (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -x hip tools/inflate_twin_check.cpp deepbedmap_amd/csrc/tiff_inflate.hip -lz -o inflate_twin_check
// Never run on a GPU machine and not part of the pytest suite: it needs no device.
#include <zlib.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

size_t tiff_inflate_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

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
  // (with no room at all zlib's uncompress decodes into a byte of its own and calls a stream of exactly one byte a success of size 0:
  // ask it with that one byte of room and count any output as "does not fit")
  uLongf got_a = (uLongf)(cap ? cap : 1);
  int rc = uncompress(a, &got_a, in, (uLong)n);
  if (cap == 0 && rc == Z_OK && got_a != 0) rc = Z_BUF_ERROR;
  const size_t got_b = tiff_inflate_twin(in, n, b, cap);
  ++g_cases;
  const bool fail_a = rc != Z_OK, fail_b = got_b == (size_t)-1;
  if (fail_a != fail_b || (!fail_a && ((size_t)got_a != got_b || memcmp(a, b, got_b) != 0))) {
    fprintf(stderr, "MISMATCH (%s, case %ld): n %zu cap %zu zlib rc %d size %lu, twin size %zd\n", what, g_cases, n, cap, rc,
            (unsigned long)got_a, (ssize_t)got_b);
    FILE* f = fopen("inflate_twin_mismatch.bin", "wb");
    if (f) { fwrite(in, 1, n, f); fclose(f); }
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
  std::vector<uint8_t> m;
  for (int k = 0; k < mutations; ++k) {
    m = stream;
    const int kind = (int)(rnd() % 8);
    size_t len = n;
    if (kind == 0) {
      len = (size_t)(rnd() % (n + 1));                                   // truncation
    } else if (kind == 1) {
      m[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));                     // one bit
    } else if (kind == 2) {
      m[rnd() % n] = (uint8_t)rnd();                                     // one byte
    } else if (kind == 3) {
      const size_t at = 2 + (size_t)(rnd() % 90);                         // inside the first block's header (a dynamic one: HLIT,
      if (at < n) m[at] ^= (uint8_t)(1u << (rnd() % 8));                 // HDIST, HCLEN, the code lengths and their repeat codes)
    } else if (kind == 4) {
      const size_t at = 2 + (size_t)(rnd() % 6);                          // the very first bytes: block type, HLIT / HDIST / HCLEN
      if (at < n) m[at] = (uint8_t)rnd();
    } else if (kind == 5) {
      const size_t at = (size_t)(rnd() % n);                              // a run of ones: extra bits forced high, long codes
      const size_t run = 1 + (size_t)(rnd() % 3);
      for (size_t i = at; i < n && i < at + run; ++i) m[i] = 0xFF;
    } else if (kind == 6) {
      const size_t at = (size_t)(rnd() % (n < 600 ? n : 600));            // early in the stream, where little has been written yet:
      m[at] |= (uint8_t)(0xF0u >> (rnd() % 5));                          // distances beyond the output
    } else {
      m[n - 1 - (size_t)(rnd() % (n < 4 ? n : 4))] ^= (uint8_t)(1u << (rnd() % 8));   // the trailer
    }
    compare(m.data(), len, caps[rnd() % 4], what);
  }
  compare(stream.data(), n / 2, decoded, what);
  // junk behind a good stream is ignored
  m = stream;
  for (int i = 0; i < 7; ++i) m.push_back((uint8_t)rnd());
  compare(m.data(), m.size(), decoded, what);
}

static std::vector<uint8_t> deflate_stream(const std::vector<uint8_t>& raw, int level, int strategy, int wbits, size_t flush_at) {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (deflateInit2(&z, level, Z_DEFLATED, wbits, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(1); }
  std::vector<uint8_t> out(deflateBound(&z, (uLong)raw.size()) + raw.size() / 4 + 64);   // (Z_FIXED on noise: 9 bits a byte)
  z.next_out = out.data();
  z.avail_out = (uInt)out.size();
  z.next_in = (Bytef*)raw.data();
  if (flush_at && flush_at < raw.size()) {
    z.avail_in = (uInt)flush_at;
    if (deflate(&z, Z_FULL_FLUSH) != Z_OK) { fprintf(stderr, "deflate (flush) failed\n"); exit(1); }
    z.avail_in = (uInt)(raw.size() - flush_at);
  } else {
    z.avail_in = (uInt)raw.size();
  }
  const int rc = deflate(&z, Z_FINISH);
  if (rc != Z_STREAM_END) { fprintf(stderr, "deflate failed (%d; level %d, strategy %d, window bits %d, %zu bytes)\n", rc, level, strategy, wbits, raw.size()); exit(1); }
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

static void check_valid(const std::vector<uint8_t>& s, const std::vector<uint8_t>& raw, const char* what) {
  std::vector<uint8_t> back(raw.size() + 1);
  if (tiff_inflate_twin(s.data(), s.size(), back.data(), raw.size()) != raw.size() || (!raw.empty() && memcmp(back.data(), raw.data(), raw.size()) != 0)) {
    fprintf(stderr, "twin does not decode '%s'\n", what);
    exit(1);
  }
}

template <typename T>
static std::vector<uint8_t> bytes_of(const std::vector<T>& f) {
  std::vector<uint8_t> raw(f.size() * sizeof(T));
  memcpy(raw.data(), f.data(), raw.size());
  return raw;
}

int main(int argc, char** argv) {
  const int mutations = 2000;
  std::vector<std::pair<std::string, std::vector<uint8_t>>> contents;
  {  // float32 Gaussian noise, a strip of 16 x 300 samples
    std::vector<float> f(16 * 300);
    for (auto& v : f) v = (float)(1000.0 * gauss());
    contents.push_back({"float32 noise", bytes_of(f)});
  }
  {  // int16 noise, 256 x 256, differenced along the rows (what predictor 2 leaves): distances up to the whole window
    std::vector<int16_t> f(256 * 256), d(256 * 256);
    for (auto& v : f) v = (int16_t)(300.0 * gauss());
    for (size_t i = 0; i < f.size(); ++i) d[i] = (i % 256) ? (int16_t)(f[i] - f[i - 1]) : f[i];
    contents.push_back({"differenced int16 noise", bytes_of(d)});
  }
  {  // a constant 256 x 256 int16 tile: distance 2, matches of 258
    std::vector<int16_t> f(256 * 256, (int16_t)-2000);
    contents.push_back({"constant tile", bytes_of(f)});
  }
  contents.push_back({"zeros", std::vector<uint8_t>(131072, 0)});   // distance 1
  {  // half constant, half noise
    std::vector<int16_t> f(128 * 256, (int16_t)-2000);
    for (size_t i = f.size() / 2; i < f.size(); ++i) f[i] = (int16_t)(300.0 * gauss());
    contents.push_back({"half constant", bytes_of(f)});
  }
  {  // differenced smooth terrain: few distinct bytes
    std::vector<uint8_t> raw(40000);
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)((i / 7) % 3);
    contents.push_back({"ramp", raw});
  }
  {  // 24 symbols with probabilities ~ 2^-k: long literal codes
    std::vector<uint8_t> raw(60000);
    for (auto& v : raw) {
      int k = 0;
      while (k < 23 && (rnd() & 1)) ++k;
      v = (uint8_t)(k * 7);
    }
    contents.push_back({"skewed symbols", raw});
  }
  contents.push_back({"one byte", std::vector<uint8_t>(1, 7)});
  contents.push_back({"nothing", std::vector<uint8_t>()});
  const int strategies[5] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
  long streams = 0;
  for (auto& c : contents) {
    const std::vector<uint8_t>& raw = c.second;
    std::vector<std::pair<std::string, std::vector<uint8_t>>> valid;
    for (int st = 0; st < 5; ++st) valid.push_back({c.first + ", strategy " + std::to_string(strategies[st]), deflate_stream(raw, 6, strategies[st], 15, 0)});
    for (int level : {0, 1, 9}) valid.push_back({c.first + ", level " + std::to_string(level), deflate_stream(raw, level, Z_DEFAULT_STRATEGY, 15, 0)});
    valid.push_back({c.first + ", window bits 9", deflate_stream(raw, 6, Z_DEFAULT_STRATEGY, 9, 0)});
    valid.push_back({c.first + ", full flush", deflate_stream(raw, 6, Z_DEFAULT_STRATEGY, 15, raw.size() * 3 / 8 + 1)});
    valid.push_back({c.first + ", level 0, full flush", deflate_stream(raw, 0, Z_DEFAULT_STRATEGY, 15, raw.size() / 2 + 1)});
    for (auto& v : valid) {
      check_valid(v.second, raw, v.first.c_str());
      torture(v.second, raw.size(), mutations, v.first.c_str());
      ++streams;
    }
  }
  // stream files: "<decoded size>:<path>" (a size of -1: the stream is one that both must refuse)
  for (int i = 1; i < argc; ++i) {
    const char* colon = strchr(argv[i], ':');
    if (!colon) { fprintf(stderr, "argument %d: expected <decoded size>:<path>\n", i); return 2; }
    const long declared = atol(argv[i]);
    FILE* f = fopen(colon + 1, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", colon + 1); return 2; }
    std::vector<uint8_t> s;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.insert(s.end(), buf, buf + got);
    fclose(f);
    const size_t decoded = declared < 0 ? 70000 : (size_t)declared;
    if (declared >= 0) {
      std::vector<uint8_t> back(decoded + 1);
      if (tiff_inflate_twin(s.data(), s.size(), back.data(), decoded) != decoded) { fprintf(stderr, "twin does not decode %s\n", colon + 1); return 1; }
    } else {
      std::vector<uint8_t> back(decoded);
      if (tiff_inflate_twin(s.data(), s.size(), back.data(), decoded) != (size_t)-1) { fprintf(stderr, "twin accepts %s\n", colon + 1); return 1; }
    }
    torture(s, decoded, mutations, colon + 1);
    ++streams;
  }
  // all-zero and all-ones inputs
  for (size_t n : {0, 1, 2, 3, 9, 64, 1000, 20000}) {
    std::vector<uint8_t> z(n, 0x00), o(n, 0xFF);
    for (size_t cap : {0, 1, 100, 70000}) {
      compare(z.data(), n, cap, "zeros");
      compare(o.data(), n, cap, "ones");
    }
  }
  printf("inflate_twin_check: %ld streams, %ld cases, %ld decoded alike, %ld rejected alike, no mismatch\n", streams, g_cases, g_ok, g_rejected);
  return 0;
}
