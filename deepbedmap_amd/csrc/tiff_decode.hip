// Decoding the blocks (strips or tiles) of a GeoTIFF on the device (dbm_tiff_decode; the host side -- header, block plan, reading the
// streams -- is deepbedmap_amd/geotiff.py; deflate blocks go through stage (a') in tiff_inflate.hip instead of stage (a)).  Replaces the reference's rasterio / GDAL reads (data_prep.py:668, :845-877;
// deepbedmap.py:164-204).  Two stages:
//
// (a) tiff_lzw_kernel -- TIFF 6.0 LZW (MSB-first codes of 9..12 bits, "early change", ClearCode 256, EndOfInformation 257: the dialect
//     of lzw_decode_one in tiff_lzw.hip), ONE WAVEFRONT PER BLOCK.  The code stream is parsed by all 64 lanes alike (every value that
//     steers the loop is wave-uniform).  The string table does not hold strings: entry e = (position in the block's OUTPUT where string e
//     was last written, its length).  That works because entry `next` is always "the previous code's string plus the first byte of the
//     current one", and those bytes lie side by side in the output: (position of the previous code's output, its length + 1).  Emitting
//     a code is a copy from earlier output, 64 bytes per pass; the KwKwK case (code == next) copies the previous string and appends its
//     first byte.  Table: 4096 x (4 + 4) bytes of LDS = 32 KiB per wave.
//     Bounds, by construction: the stream is read only at byte indices < n (a code that would need a byte at or past n ends the
//     decoding, as in the host decoder); every copy is preceded by outn + len <= cap; a table entry (pos, len) is only ever read for
//     258 <= code < next, and every such entry was written since the last ClearCode with pos + len <= outn at that time, so the copy's
//     source lies inside what has been written.  Every loop ends: one iteration consumes at least 9 bits of the stream, a copy runs over
//     len <= cap bytes.  Nothing is retried, nothing spins.
//     lzw_decode_lanes is __host__ __device__: with (lane, lanes) = (0, 1) it is the host twin (tiff_lzw_decode_twin) that the
//     stand-alone robustness program (tools/lzw_twin_check.cpp) runs against lzw_decode_one.
// (b) tiff_rows_kernel -- one workgroup per block row: undo the predictor in place in the decoded bytes (2: wrapping prefix sum over
//     the row's samples in their own width; 3: wrapping prefix sum over the row's W * bytes bytes, then the big-endian byte planes are
//     gathered into little-endian samples), convert to float32 as numpy.astype does, write at the block's place in the output plane;
//     samples outside the plane (tile padding, the part of a block outside the window) are dropped.
#include "model.h"
#include "data_prims.h"

namespace {

constexpr int ROW_THREADS = 256;

// Decodes src[0, n) into dst[0, cap).  Returns the decoded size, or (size_t)-1 on the conditions lzw_decode_one returns it: a first code
// above 255, a code above `next`, more output than cap.  A stream that ends without EndOfInformation is not an error here (the caller
// compares the size).  tpos / tlen: 4096 entries each, uninitialised.  All lanes of the wave call it with the same arguments but `lane`.
__host__ __device__ inline size_t lzw_decode_lanes(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, uint32_t* tpos, uint32_t* tlen,
                                                   uint32_t lane, uint32_t lanes) {
  size_t pos = 0, outn = 0;
  uint64_t acc = 0;        // the low `have` bits are the stream's next bits, most significant first
  uint32_t have = 0, width = 9, next = 258, oldpos = 0, oldlen = 0;
  bool have_old = false;
  for (;;) {
    if (have < width) {    // (have <= 11: four more bytes fit)
      if (pos >= n) break;
      // up to four bytes in one go, as four independent loads: indices clamped to n - 1, the surplus shifted out again
      const size_t last = n - 1;
      const uint32_t take = n - pos < 4 ? (uint32_t)(n - pos) : 4u;
      const uint32_t w = (uint32_t)src[pos] << 24 | (uint32_t)src[pos + 1 < last ? pos + 1 : last] << 16 |
                         (uint32_t)src[pos + 2 < last ? pos + 2 : last] << 8 | (uint32_t)src[pos + 3 < last ? pos + 3 : last];
      acc = (acc << (8 * take)) | (uint64_t)(w >> (8 * (4 - take)));
      have += 8 * take;
      pos += take;
      if (have < width) break;   // (only at the end of the stream: the host decoder stops where a byte at or past n would be needed)
    }
    have -= width;
    const uint32_t code = (uint32_t)(acc >> have) & ((1u << width) - 1u);
    if (code == 257) break;
    if (code == 256) { width = 9; next = 258; have_old = false; continue; }
    if (!have_old) {
      if (code > 255) return (size_t)-1;
      if (outn >= cap) return (size_t)-1;
      if (lane == 0) dst[outn] = (uint8_t)code;
      oldpos = (uint32_t)outn; oldlen = 1;
      ++outn;
      have_old = true;
      lanes_fence();
      continue;
    }
    uint32_t spos = 0, slen = 1;
    const bool literal = code < 256;
    bool kwkwk = false;
    if (!literal) {
      if (code < next) { spos = tpos[code]; slen = tlen[code]; }
      else if (code == next) { spos = oldpos; slen = oldlen + 1; kwkwk = true; }
      else return (size_t)-1;
    }
    if (outn + slen > cap) return (size_t)-1;
    // source [spos, spos + slen) ends at or before outn (KwKwK: its last byte is the first one again): no lane reads what another writes
    for (uint32_t i = lane; i < slen; i += lanes)
      dst[outn + i] = literal ? (uint8_t)code : dst[spos + ((kwkwk && i == oldlen) ? 0u : i)];
    if (next < 4096) {
      if (lane == 0) { tpos[next] = oldpos; tlen[next] = oldlen + 1; }
      ++next;
      if (next == 511 || next == 1023 || next == 2047) ++width;
    }
    oldpos = (uint32_t)outn; oldlen = slen;
    outn += slen;
    lanes_fence();
  }
  return outn;
}

__global__ __launch_bounds__(64) void tiff_lzw_kernel(StreamDecodeLaunch a) {
  __shared__ uint32_t tpos[4096];
  __shared__ uint32_t tlen[4096];
  const long b = blockIdx.x;
  const long* e = a.blocks + 8 * b;
  const size_t want = (size_t)(a.whole_rows ? a.whole_rows : e[2]) * (size_t)a.row_bytes;   // <= block_stride (checked by the caller)
  const size_t got = lzw_decode_lanes(a.streams + e[0], (size_t)e[1], a.stage + b * a.block_stride, want, tpos, tlen, threadIdx.x, 64u);
  if (threadIdx.x == 0) a.status[b] = got == (size_t)-1 ? 1 : (got != want ? 2 : 0);
}

__device__ inline unsigned long long load_le(const uint8_t* p, int w) {
  switch (w) {
    case 1: return *p;
    case 2: return *(const uint16_t*)p;
    case 4: return *(const uint32_t*)p;
    default: return *(const unsigned long long*)p;
  }
}
__device__ inline void store_le(uint8_t* p, int w, unsigned long long v) {
  switch (w) {
    case 1: *p = (uint8_t)v; break;
    case 2: *(uint16_t*)p = (uint16_t)v; break;
    case 4: *(uint32_t*)p = (uint32_t)v; break;
    default: *(unsigned long long*)p = v; break;
  }
}

// workgroup idx -> (block b, row r of the block).  Rows of a block are independent: the predictors run along rows only.
__global__ __launch_bounds__(ROW_THREADS) void tiff_rows_kernel(TiffDecodeLaunch a) {
  const long b = (long)blockIdx.x / a.block_h, r = (long)blockIdx.x - b * a.block_h;
  const long* e = a.blocks + 8 * b;
  const long orow = e[3] + r;
  if (r >= e[2] || orow < 0 || orow >= a.out_h) return;   // (uniform in the workgroup)
  uint8_t* row = (a.staged ? a.stage + b * a.block_stride : a.stage + e[0]) + r * (long)a.block_w * a.bytes;
  const int tid = threadIdx.x;
  if (a.predictor != 1) {
    const int w = a.predictor == 2 ? a.bytes : 1;                        // element width of the running sum
    const long count = a.predictor == 2 ? a.block_w : (long)a.block_w * a.bytes;
    unsigned long long carry = 0;
    for (long i0 = 0; i0 < count; i0 += ROW_THREADS) {
      const long i = i0 + tid;
      const unsigned long long v = i < count ? load_le(row + i * w, w) : 0ull;
      unsigned long long total;
      const unsigned long long before = carry + block_exscan<ROW_THREADS>(v, &total);
      if (i < count) store_le(row + i * w, w, before + v);   // (the store keeps the low 8 w bits: the sum wraps in the sample's width)
      carry += total;
    }
    __syncthreads();   // the row's bytes are visible to the whole workgroup (the scan's own barriers come before its round's stores)
  }
  const long ocol0 = e[4];
  uint32_t* out = (uint32_t*)a.out + orow * a.out_w;
  for (long c = tid; c < a.block_w; c += ROW_THREADS) {
    const long oc = ocol0 + c;
    if (oc < 0 || oc >= a.out_w) continue;
    unsigned long long raw;
    if (a.predictor == 3) {   // byte plane k holds byte k of every sample, most significant plane first
      raw = 0;
      for (int k = 0; k < a.bytes; ++k) raw = (raw << 8) | row[(long)k * a.block_w + c];
    } else {
      raw = load_le(row + c * a.bytes, a.bytes);
    }
    uint32_t bits;
    switch (a.sample_type) {
      case 0: bits = __float_as_uint((float)(uint8_t)raw); break;
      case 1: bits = __float_as_uint((float)(int16_t)(uint16_t)raw); break;
      case 2: bits = __float_as_uint((float)(uint16_t)raw); break;
      case 3: bits = __float_as_uint((float)(int32_t)(uint32_t)raw); break;
      case 4: bits = (uint32_t)raw; break;                                    // float32: the bits, NaN payloads included
      default: bits = __float_as_uint((float)__longlong_as_double((long long)raw)); break;
    }
    out[oc] = bits;
  }
}

}  // namespace

void launch_block_lzw(const StreamDecodeLaunch& a, hipStream_t s) {
  if (a.n_blocks <= 0) return;
  hipLaunchKernelGGL(tiff_lzw_kernel, dim3((unsigned)a.n_blocks), dim3(64), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_tiff_rows(const TiffDecodeLaunch& a, hipStream_t s) {
  const long groups = (long)a.n_blocks * a.block_h;
  if (groups <= 0) return;
  DBM_CHECK(groups < (1L << 31), "dbm_tiff_decode: more than 2^31 block rows in one call");
  hipLaunchKernelGGL(tiff_rows_kernel, dim3((unsigned)groups), dim3(ROW_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

size_t tiff_lzw_decode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) {
  std::vector<uint32_t> tab(2 * 4096);
  return lzw_decode_lanes(src, n, dst, cap, tab.data(), tab.data() + 4096, 0u, 1u);
}
