// A resident 8-bit image -> the bands of a PNG's zlib stream (dbm_png_encode, api_data.hip) and the same bytes from a host image
// (dbm_png_encode_host, here).  Reference: deepbedmap.py:758-775 and paper_figures.py:692-699 end in `fig.savefig(...png)` through GMT;
// this file is the part of that step that touches every pixel.  The container (signature, IHDR, IDAT, IEND, CRC-32) is the host
// shim's, deepbedmap_amd/relief.py; DESIGN.md 6n has the rules statement by statement.
//
// Bands.  The image (H rows of row_bytes = W * channels bytes, 8 bits per sample) is cut into bands of band_rows rows; band b holds
// rows b * band_rows ..., the last band is short.  A band's bytes are, row after row, ONE filter-type byte and the row's row_bytes
// filtered bytes -- what PNG calls the filtered scanlines, so the bands one behind the other are the data a PNG's zlib stream holds.
//
// Filters (PNG 1.2, 6.2 .. 6.4; bpp = channels bytes per pixel; all arithmetic modulo 256), byte x of row r:
//   0 None  Raw(r, x)
//   1 Sub   Raw(r, x) - Raw(r, x - bpp), Raw(r, x - bpp) = 0 for x < bpp
//   2 Up    Raw(r, x) - Raw(r - 1, x),   Raw(-1, x) = 0
// computed from the RAW image: Up reads the row above also where that row belongs to the band before.  One filter type per image.
//
// Each band then becomes one segment of the zlib stream (deflate_encode.hip, framing 1; the image's last band framing 2): a segment
// starts with an empty hash table, so bands are encoded independently, one wavefront each, and the host writes 78 01, the segments,
// and the Adler-32 joined from the segments' own sums.
//
// png_band_byte is the one text of the rule: the kernel calls it for four bytes per thread, the host writer for every byte.
#include "api_common.h"
#include "data_prims.h"
#include <cstring>
#include <thread>

namespace {

constexpr int PNG_THREADS = 256;
constexpr long PNG_BYTES_PER_GROUP = 16384;   // of a band, per workgroup of the filter kernel

// byte k of the band whose first image row is r0 (k < rows * (row_bytes + 1))
__host__ __device__ inline uint8_t png_band_byte(const uint8_t* image, long row_bytes, int bpp, int filter, long r0, long k) {
  const long r = r0 + k / (row_bytes + 1), j = k % (row_bytes + 1);
  if (j == 0) return (uint8_t)filter;
  const long x = j - 1;
  const uint8_t raw = image[r * row_bytes + x];
  if (filter == 1) return (uint8_t)(raw - (x >= bpp ? image[r * row_bytes + x - bpp] : (uint8_t)0));
  if (filter == 2) return (uint8_t)(raw - (r > 0 ? image[(r - 1) * row_bytes + x] : (uint8_t)0));
  return raw;
}

// workgroup g of band b writes the band's bytes [g * PNG_BYTES_PER_GROUP, ...): four bytes per thread and store (raw + b * raw_stride
// is 16-byte aligned; the bytes of the last word beyond the band are zero and lie inside raw_stride)
__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(PngFilterLaunch a) {
  const long b = blockIdx.x / a.groups_per_band, g = blockIdx.x % a.groups_per_band;
  const long r0 = (a.first_band + b) * a.band_rows;
  const long rows = a.H - r0 < a.band_rows ? a.H - r0 : (long)a.band_rows;
  const long n = rows * (a.row_bytes + 1);
  const long end = (g + 1) * PNG_BYTES_PER_GROUP < n ? (g + 1) * PNG_BYTES_PER_GROUP : n;
  uint32_t* out = (uint32_t*)(a.raw + b * a.raw_stride);
  for (long k = g * PNG_BYTES_PER_GROUP + 4L * threadIdx.x; k < end; k += 4L * PNG_THREADS) {
    uint32_t word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k + q < n) word |= (uint32_t)png_band_byte(a.image, a.row_bytes, a.bpp, a.filter, r0, k + q) << (8 * q);
    out[k >> 2] = word;
  }
}

}  // namespace

unsigned png_groups_per_band(long band_bytes) { return (unsigned)((band_bytes + PNG_BYTES_PER_GROUP - 1) / PNG_BYTES_PER_GROUP); }

void launch_png_filter(const PngFilterLaunch& a, hipStream_t s) {
  if (a.n_bands <= 0) return;
  const long groups = (long)a.n_bands * a.groups_per_band;
  DBM_CHECK(groups < (1L << 31), "dbm_png_encode: more than 2^31 workgroups in one call");
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)groups), dim3(PNG_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

PngWorkspace png_workspace(void* ws, size_t n_bands, size_t raw_stride, size_t slot_cap, size_t words_per_band) {
  Carver carve(ws);
  PngWorkspace w;
  w.raw = carve.take<uint8_t>(n_bands * raw_stride);
  w.slots = carve.take<uint8_t>(n_bands * slot_cap);
  w.words = (uint32_t*)carve.take<uint8_t>(n_bands * words_per_band);
  w.segment_words = carve.take<uint32_t>(2 * n_bands);
  w.bytes = carve.bytes();
  return w;
}

// what dbm_png_encode and dbm_png_encode_host refuse alike (status 1); returns the number of bands of the image
long png_check_arguments(const char* who, const void* image, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                         const void* out, size_t out_capacity, const void* sizes, const void* adlers) {
  const std::string w(who);
  DBM_CHECK(image != nullptr, w + ": NULL image");
  DBM_CHECK(H >= 1 && W >= 1, w + ": empty image");
  DBM_CHECK(channels == 1 || channels == 3 || channels == 4, w + ": channels must be 1 (grey), 3 (RGB) or 4 (RGBA)");
  DBM_CHECK(H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31), w + ": H W must stay below 2^31 pixels");
  DBM_CHECK(filter >= 0 && filter <= 2, w + ": filter must be 0 (None), 1 (Sub) or 2 (Up)");
  DBM_CHECK(band_rows >= 1, w + ": band_rows must be at least 1");
  const long rows = band_rows < H ? (long)band_rows : H;
  DBM_CHECK(rows * (W * channels + 1) < (1L << 31), w + ": a band must hold less than 2^31 bytes");
  const long bands = (H + band_rows - 1) / band_rows;
  DBM_CHECK(first_band >= 0 && n_bands >= 0 && first_band + (long)n_bands <= bands, w + ": the band range lies outside the image's " +
                                                                                       std::to_string(bands) + " bands");
  DBM_CHECK(n_bands == 0 || (out != nullptr && sizes != nullptr && adlers != nullptr), w + ": NULL output, sizes or adlers");
  const size_t worst = (deflate_slot((size_t)(rows * (W * channels + 1))) + 1) & ~(size_t)1;
  DBM_CHECK(out_capacity / worst >= (size_t)n_bands, w + ": the output holds " + std::to_string(out_capacity) + " bytes, the worst case of " +
                                                         std::to_string(n_bands) + " bands is " + std::to_string((size_t)n_bands * worst));
  return bands;
}

extern "C" int dbm_png_encode_host(const void* image, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                                   void* out, size_t out_capacity, size_t* sizes, uint32_t* adlers, int nthreads) {
  DBM_API_BEGIN(nullptr)
  const long bands = png_check_arguments("dbm_png_encode_host", image, H, W, channels, filter, band_rows, first_band, n_bands, out, out_capacity,
                                         sizes, adlers);
  if (n_bands == 0) return 0;
  const long row_bytes = W * channels;
  const size_t band_bytes = (size_t)(band_rows < H ? band_rows : H) * (size_t)(row_bytes + 1), slot_cap = deflate_slot(band_bytes);
  if (nthreads < 1) nthreads = 1;
  if (nthreads > n_bands) nthreads = n_bands;
  std::vector<uint8_t> slots((size_t)n_bands * slot_cap);
  auto work = [&](int t0) {
    std::vector<uint16_t> table(16384);
    std::vector<uint8_t> raw(band_bytes);
    for (int t = t0; t < n_bands; t += nthreads) {
      const long b = first_band + t, r0 = b * band_rows;
      const long rows = H - r0 < band_rows ? H - r0 : (long)band_rows;
      const size_t n = (size_t)rows * (size_t)(row_bytes + 1);
      for (size_t k = 0; k < n; ++k) raw[k] = png_band_byte((const uint8_t*)image, row_bytes, channels, filter, r0, (long)k);
      sizes[t] = deflate_encode_twin(raw.data(), n, slots.data() + (size_t)t * slot_cap, slot_cap, table.data(), b == bands - 1 ? 2 : 1, adlers + t);
    }
  };
  std::vector<std::thread> th;
  for (int i = 1; i < nthreads; ++i) th.emplace_back(work, i);
  work(0);
  for (auto& t : th) t.join();
  size_t at = 0;   // dbm_png_encode's packing: every segment at the next even offset, an odd one followed by a zero byte
  for (int t = 0; t < n_bands; ++t) {
    if (sizes[t] == 0) throw DbmError(12, "dbm_png_encode_host: band " + std::to_string(first_band + t) + ": its deflate segment does not fit the slot");
    std::memcpy((uint8_t*)out + at, slots.data() + (size_t)t * slot_cap, sizes[t]);
    at += sizes[t];
    if (at & 1) ((uint8_t*)out)[at++] = 0;
  }
  DBM_API_END
}
