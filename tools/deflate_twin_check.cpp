// Stand-alone check of the device deflate encoder's loop on the CPU.  deflate_encode_lanes (deflate_encode.hip) is
// __host__ __device__; dbm_deflate_encode_blocks runs it with one lane.  From a fixed seed this program encodes float32 noise, a
// constant block, a half-constant block, a ramp and uniform random bytes -- each also after HDF5's shuffle over the block -- at lengths
// 0, 1, 2, 3, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769, 65536 and 262144, and demands for every case that the stream starts 78 01,
// stays within n + n / 8 + 16 bytes and that both zlib's `uncompress` and dbm_inflate (the device inflater's loop with one lane) return
// the input; then, with capacities equal to, one below and far below the encoded size, that the encoder reports failure exactly where
// the stream does not fit, writes the same bytes where it does and writes nothing outside its buffer.  Built with AddressSanitizer and
// UBSan on the host side, every buffer exactly as large as declared (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -x hip tools/deflate_twin_check.cpp deepbedmap_amd/csrc/deflate_encode.hip deepbedmap_amd/csrc/tiff_inflate.hip \
//         -lz -o deflate_twin_check
// Never run on a GPU machine and not part of the pytest suite: it needs no device.
#include <zlib.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int dbm_deflate_encode_blocks(const void* blocks, size_t block_bytes, int nblocks, void* out, size_t out_stride, size_t* out_sizes,
                                         int nthreads);
extern "C" int dbm_inflate(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return g_state;
}
static double gauss() {
  const double u = ((rnd() >> 11) + 1.0) / 9007199254740993.0, v = (rnd() >> 11) / 9007199254740992.0;
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

static long g_cases = 0, g_decoded = 0, g_refused = 0;
static size_t g_raw = 0, g_encoded = 0;

static void fail(const char* what, size_t n, size_t cap, const char* why) {
  fprintf(stderr, "MISMATCH (%s): n %zu cap %zu: %s\n", what, n, cap, why);
  exit(1);
}

// the encoder on src[0, n) with `cap` bytes of room, into a heap buffer of exactly cap bytes; returns the size (0: refused).  `expect`:
// the stream of an earlier call with room enough, or null.
static size_t encode(const uint8_t* src, size_t n, size_t cap, const char* what, const std::vector<uint8_t>* expect, std::vector<uint8_t>* keep) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);   // (an exact copy: a read at or past n is a heap overflow)
  if (n) memcpy(in, src, n);
  uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
  memset(out, 0xAA, cap ? cap : 1);
  size_t size = 0;
  const int rc = dbm_deflate_encode_blocks(in, n, 1, out, cap, &size, 1);
  ++g_cases;
  if (rc != 0 && rc != 2) fail(what, n, cap, "an unexpected status");
  if (rc == 2) {
    if (size != 0) fail(what, n, cap, "refused, but a size is reported");
    ++g_refused;
  } else {
    if (size < 8 || size > cap || out[0] != 0x78 || out[1] != 0x01) fail(what, n, cap, "no zlib stream of the declared size");
    if (expect && (size != expect->size() || memcmp(out, expect->data(), size) != 0)) fail(what, n, cap, "the stream depends on the capacity");
    uint8_t* back = (uint8_t*)malloc(n ? n : 1);
    uLongf got = (uLongf)n;
    if (uncompress(back, &got, out, (uLong)size) != Z_OK || got != n || (n && memcmp(back, in, n) != 0)) fail(what, n, cap, "zlib does not return the input");
    memset(back, 0, n ? n : 1);
    size_t twin = 0;
    if (dbm_inflate(out, size, back, n, &twin) != 0 || twin != n || (n && memcmp(back, in, n) != 0)) fail(what, n, cap, "dbm_inflate does not return the input");
    free(back);
    if (keep) keep->assign(out, out + size);
    ++g_decoded;
  }
  free(in);
  free(out);
  return size;
}

static void check(const std::vector<uint8_t>& raw, const char* what) {
  const size_t n = raw.size(), slot = n + n / 8 + 16;
  std::vector<uint8_t> stream;
  const size_t size = encode(raw.data(), n, slot, what, nullptr, &stream);   // the slot of the device path
  if (size == 0) fail(what, n, slot, "refused with the full slot");
  g_raw += n;
  g_encoded += size;
  const size_t caps[6] = {size, size - 1, size / 2, (size_t)2, (size_t)1, (size_t)0};
  for (size_t k = 0; k < 6; ++k) {
    const size_t got = encode(raw.data(), n, caps[k], what, &stream, nullptr);
    if ((got != 0) != (caps[k] >= size)) fail(what, n, caps[k], "accepted or refused at the wrong capacity");
  }
}

// HDF5's shuffle over the whole buffer of 4-byte elements: byte k of element i goes to k * count + i; a trailing partial element stays
static std::vector<uint8_t> shuffle4(const std::vector<uint8_t>& raw) {
  std::vector<uint8_t> out(raw);
  const size_t count = raw.size() / 4;
  for (size_t i = 0; i < count; ++i)
    for (size_t k = 0; k < 4; ++k) out[k * count + i] = raw[4 * i + k];
  return out;
}

int main() {
  const size_t whole = 256 * 256;   // float32 samples: 262144 bytes
  std::vector<std::pair<std::string, std::vector<uint8_t>>> contents;
  auto add = [&](const char* name, const void* data) {
    std::vector<uint8_t> raw(whole * 4);
    memcpy(raw.data(), data, raw.size());
    contents.push_back({name, raw});
  };
  {
    std::vector<float> f(whole);
    for (auto& v : f) v = (float)(300.0 * gauss());
    add("noise", f.data());
  }
  {
    std::vector<float> f(whole, -2000.0f);
    add("constant", f.data());
  }
  {
    std::vector<float> f(whole, -2000.0f);
    for (size_t i = whole / 2; i < whole; ++i) f[i] = (float)(300.0 * gauss());
    add("half constant", f.data());
  }
  {
    std::vector<float> f(whole);
    for (size_t i = 0; i < whole; ++i) f[i] = (float)(3 * (i % 256) + (i / 256));
    add("ramp", f.data());
  }
  {
    std::vector<uint32_t> f(whole);
    for (auto& v : f) v = (uint32_t)rnd();
    add("uniform random bytes", f.data());
  }
  const size_t lengths[15] = {0, 1, 2, 3, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769, 65536, 262144};
  for (auto& c : contents) {
    for (int shuffled = 0; shuffled <= 1; ++shuffled) {
      const std::string name = c.first + (shuffled ? " shuffled" : "");
      for (size_t len : lengths) {
        std::vector<uint8_t> raw(c.second.begin(), c.second.begin() + (long)len);
        check(shuffled ? shuffle4(raw) : raw, name.c_str());
      }
    }
  }
  printf("deflate_twin_check: %ld cases, %ld streams decoded back by zlib and dbm_inflate, %ld refused for lack of room, no mismatch; %zu bytes in, %zu out\n",
         g_cases, g_decoded, g_refused, g_raw, g_encoded);
  return 0;
}
