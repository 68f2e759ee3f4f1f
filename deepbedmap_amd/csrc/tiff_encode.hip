// Encoding the blocks (strips or tiles) of a GeoTIFF on the device (dbm_tiff_encode; the host side -- container, tags, batching -- is
// deepbedmap_amd/geotiff.py: write_geotiff_resident).  The counterpart of tiff_decode.hip for the product's own output (reference
// deepbedmap.py:749-756 -> data_prep.py:779-834: GeoTIFF, int16, tiled, compress=lzw).  Three launches:
//
// (a) tiff_blocks_kernel -- one workgroup per block row: the float32 plane's samples as the block's raw bytes in a staging buffer.
//     int16: the cast of f32_to_i16_kernel (dbm_cast_i16, kernels.h: NumPy's astype); float32: the bits.  Tiles are whole, positions
//     right of or below the plane are zero bytes; the last strip holds only the rows that exist.  Predictor 2: d[0] = s[0], d[c] =
//     s[c] - s[c - 1] over the block's row INCLUDING its padding columns, wrapping in the sample's own width (uint16 / the 32-bit
//     patterns): the inverse of what tiff_rows_kernel (tiff_decode.hip) undoes.  Every thread forms s[c] and s[c - 1] itself: no scan.
// (b) tiff_lzw_encode_kernel -- TIFF 6.0 LZW (the dialect and the rules of lzw_encode_one in tiff_lzw.hip: MSB-first codes of 9..12
//     bits, the early change at 512 / 1024 / 2048, ClearCode when entry 4093 has been added, the trailing entry before
//     EndOfInformation), ONE WAVEFRONT PER BLOCK.  Every value that steers the loop is wave-uniform.  The string table is open
//     addressing in LDS: 8192 slots of one 32-bit word = (20-bit key = prefix code << 8 | byte) << 12 | 12-bit code, all ones = empty
//     (no entry has code 4095), 32 KiB per wave.  The slots form 128 rows of 64: the 64 lanes read one row at once and ballot for a
//     match and for the first empty slot; a key that is not found is inserted into that first empty slot, so lookup and insert agree
//     by construction; a full row sends both on to the next row.  The output of LZW is determined by its rule, not by the table's
//     layout, so the bytes equal lzw_encode_one's.
//     The input is held 64 bytes at a time, one byte per lane (the next 64 are loaded while these are consumed).
//     Bounds, by construction: the input is read at indices < n only (the chunk loads are guarded by i < n); every output store is
//     preceded by `count < cap` -- on overflow the flag is set, the loop ends, 0 is returned (status word 1) and nothing is written at
//     or past cap; each iteration of the main loop consumes exactly one input byte; the probe visits at most all 128 rows once, and as
//     the table holds at most 3836 of 8192 slots it ends at an empty slot (should it ever not, the block fails like an overflow).
//     Nothing is retried, nothing spins.
//     lzw_encode_lanes is __host__ __device__: with (lane, lanes) = (0, 1) it is the host twin (tiff_lzw_encode_twin) that the
//     stand-alone program tools/lzw_encode_twin_check.cpp compares with dbm_lzw_encode_tiles.  Only the lane primitives differ between
//     the two compilations: probe_row (ballot / readlane against a loop over the row's 64 slots) and chunk_byte (readlane against a
//     load of the byte itself).
// (c) tiff_pack_kernel -- the streams from their slots (stride = capacity = block_bytes * 3 / 2 + 64, the host encoder's bound) to the
//     even-aligned offsets the host computed from the downloaded sizes; one D2H copy then brings them over.
#include "model.h"
#include "data_prims.h"

namespace {

constexpr int ROW_THREADS = 256;
constexpr uint32_t LZW_SLOTS = 8192, LZW_ROWS = LZW_SLOTS / 64, LZW_EMPTY = 0xFFFFFFFFu;
constexpr int PACK_PARTS = 16;

// ---- lane primitives: the only code that differs between the device and the host twin ----
// One row of the table (64 slots) against `key`: true and the entry's code if a slot holds the key; else `empty` = index in the row of
// its first empty slot, or 64 if the row is full.
__host__ __device__ inline bool probe_row(const uint32_t* row, uint32_t key, uint32_t lane, uint32_t& code, uint32_t& empty) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t w = row[lane];
  const unsigned long long match = __ballot((w >> 12) == key && w != LZW_EMPTY);
  if (match) {
    code = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)__builtin_ctzll(match)) & 0xFFFu;
    return true;
  }
  const unsigned long long free_slots = __ballot(w == LZW_EMPTY);
  empty = free_slots ? (uint32_t)__builtin_ctzll(free_slots) : 64u;
  return false;
#else
  (void)lane;
  empty = 64u;
  for (uint32_t k = 0; k < 64u; ++k) {
    const uint32_t w = row[k];
    if (w == LZW_EMPTY) {
      if (empty == 64u) empty = k;
    } else if ((w >> 12) == key) {
      code = w & 0xFFFu;
      return true;
    }
  }
  return false;
#endif
}

// Input byte i (< n).  Device: the lanes hold src[i & ~63 ...] one byte each in `chunk`.
__host__ __device__ inline uint32_t chunk_byte(const uint8_t* src, size_t i, uint32_t chunk) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)src;
  return (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)(i & 63));
#else
  (void)chunk;
  return src[i];
#endif
}

// MSB-first bit packer of lzw_encode_one's BitWriter; lane 0 stores.  A byte is stored only while count < cap.
struct LaneBitWriter {
  uint8_t* out;
  size_t cap, count;
  uint32_t acc, bits, lane;
  bool overflow;
  __host__ __device__ inline void emit(uint32_t byte) {
    if (count < cap) {
      if (lane == 0) out[count] = (uint8_t)byte;
    } else {
      overflow = true;
    }
    ++count;
  }
  // bits <= 7 before and width <= 12: at most 19 bits in use, at most two whole bytes leave (BitWriter's `while (bits >= 8)`)
  __host__ __device__ inline void put(uint32_t code, uint32_t width) {
    acc = ((acc << width) | code) & 0xFFFFFu;
    bits += width;
    if (bits >= 8) {
      bits -= 8;
      emit(acc >> bits);
    }
    if (bits >= 8) {
      bits -= 8;
      emit(acc >> bits);
    }
  }
  __host__ __device__ inline void flush() {
    if (bits > 0) {
      emit(acc << (8 - bits));
      bits = 0;
    }
  }
};

__host__ __device__ inline void table_reset(uint32_t* table, uint32_t lane, uint32_t lanes) {
#pragma unroll 8
  for (uint32_t i = lane; i < LZW_SLOTS; i += lanes) table[i] = LZW_EMPTY;
  lanes_fence();
}

// Encodes src[0, n) into dst[0, cap).  Returns the encoded size, or 0 if cap is too small (as lzw_encode_one).  table: LZW_SLOTS words,
// uninitialised.  All lanes of the wave call it with the same arguments but `lane`.
__host__ __device__ inline size_t lzw_encode_lanes(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, uint32_t* table, uint32_t lane,
                                                   uint32_t lanes) {
  LaneBitWriter w{dst, cap, 0, 0u, 0u, lane, false};
  uint32_t width = 9, next = 258;
  table_reset(table, lane, lanes);
  w.put(256u, width);
  if (n == 0) {
    w.put(257u, width);
    w.flush();
    return w.overflow ? 0 : w.count;
  }
  // the 64 bytes in use and the 64 behind them, one byte per lane (the host twin's single lane reads the byte itself in chunk_byte)
  uint32_t chunk = lane < n ? src[lane] : 0u;
  uint32_t ahead = (size_t)64 + lane < n ? src[(size_t)64 + lane] : 0u;
  uint32_t omega = chunk_byte(src, 0, chunk);
#pragma unroll 1
  for (size_t i = 1; i < n; ++i) {
    if ((i & 63) == 0) {
      chunk = ahead;
      ahead = i + 64 + lane < n ? src[i + 64 + lane] : 0u;
    }
    const uint32_t k = chunk_byte(src, i, chunk);
    const uint32_t key = (omega << 8) | k;
    uint32_t row = (key * 2654435761u) >> 25;   // 7 bits: one of LZW_ROWS rows
    uint32_t code = 0, empty = 64u;
    bool found = false;
#pragma unroll 1
    for (uint32_t visited = 0; visited < LZW_ROWS; ++visited) {
      found = probe_row(table + row * 64u, key, lane, code, empty);
      if (found || empty < 64u) break;
      row = (row + 1u) & (LZW_ROWS - 1u);
    }
    if (found) {
      omega = code;
      continue;
    }
    if (empty >= 64u) {   // (every row full: impossible with at most 3836 entries; fails like an overflow, nothing is inserted)
      w.overflow = true;
      break;
    }
    w.put(omega, width);
    if (lane == 0) table[row * 64u + empty] = (key << 12) | next;
    lanes_fence();
    ++next;
    // the points of lzw_encode_one (TIFF 6.0 section 13, "early change"; ClearCode when entry 4093 has been added)
    if (next == 4094u) {
      w.put(256u, width);
      table_reset(table, lane, lanes);
      width = 9;
      next = 258;
    } else if (next == 512u || next == 1024u || next == 2048u) {
      ++width;
    }
    omega = k;
    if (w.overflow) break;   // a store was refused: the loop ends
  }
  if (w.overflow) return 0;
  w.put(omega, width);
  // the decoder adds a table entry after this code as well: the EndOfInformation code may need the wider field
  ++next;
  if (next == 4094u) {
    w.put(256u, width);
    width = 9;
  } else if (next == 512u || next == 1024u || next == 2048u) {
    ++width;
  }
  w.put(257u, width);
  w.flush();
  return w.overflow ? 0 : w.count;
}

// rows that block `gb` (index in the image) holds, and its row / column of blocks
__device__ inline long block_rows(const TiffEncodeLaunch& a, long gb, long& by, long& bx) {
  by = gb / a.blocks_x;
  bx = gb - by * a.blocks_x;
  const long left = a.H - by * a.block_h;
  return a.tiled || left > a.block_h ? (long)a.block_h : left;
}

__device__ inline uint32_t sample_bits(const TiffEncodeLaunch& a, long prow, long pcol) {
  if (prow >= a.H || pcol >= a.W) return 0u;   // tile padding
  const float x = a.plane[prow * a.W + pcol];
  return a.sample_type == 1 ? (uint32_t)(uint16_t)dbm_cast_i16(x) : __float_as_uint(x);
}

// workgroup idx -> (block b of the call, row r of the block)
__global__ __launch_bounds__(ROW_THREADS) void tiff_blocks_kernel(TiffEncodeLaunch a) {
  const long b = (long)blockIdx.x / a.block_h, r = (long)blockIdx.x - b * a.block_h;
  long by, bx;
  const long rows = block_rows(a, a.first + b, by, bx);
  if (r >= rows) return;   // (uniform in the workgroup: a short last strip has no such row)
  const long prow = by * a.block_h + r, pcol0 = bx * a.block_w;
  uint8_t* out = a.raw + b * a.raw_stride + r * (long)a.block_w * a.bytes;   // (raw_stride is a multiple of 16: aligned for the sample)
  for (long c = threadIdx.x; c < a.block_w; c += ROW_THREADS) {
    uint32_t v = sample_bits(a, prow, pcol0 + c);
    if (a.predictor == 2 && c > 0) v -= sample_bits(a, prow, pcol0 + c - 1);
    if (a.bytes == 2) ((uint16_t*)out)[c] = (uint16_t)v;   // (the store keeps the low 16 bits: the difference wraps in the sample's width)
    else ((uint32_t*)out)[c] = v;
  }
}

__global__ __launch_bounds__(64) void tiff_lzw_encode_kernel(TiffEncodeLaunch a) {
  __shared__ uint32_t table[LZW_SLOTS];
  const long b = blockIdx.x;
  long by, bx;
  const size_t n = (size_t)block_rows(a, a.first + b, by, bx) * (size_t)a.block_w * (size_t)a.bytes;   // <= raw_stride
  const size_t got = lzw_encode_lanes(a.raw + b * a.raw_stride, n, a.slots + (size_t)b * a.slot_cap, a.slot_cap, table, threadIdx.x, 64u);
  if (threadIdx.x == 0) {
    a.result[2 * b] = (uint32_t)got;             // (slot_cap < 2^32: block_bytes < 2^31)
    a.result[2 * b + 1] = got == 0 ? 1u : 0u;    // the status word: 1 = the stream did not fit its slot
  }
}

// table: per block {offset in `packed`, size}; the stream of block b lies at src + b * src_stride.  An odd size is followed by one zero
// byte (the next offset is even).
__global__ __launch_bounds__(ROW_THREADS) void tiff_pack_kernel(const uint8_t* __restrict__ src, size_t src_stride, const unsigned long long* __restrict__ table,
                                                                uint8_t* __restrict__ packed) {
  const size_t b = blockIdx.x;
  const unsigned long long off = table[2 * b], size = table[2 * b + 1];
  const uint8_t* s = src + b * src_stride;
  for (unsigned long long i = (unsigned long long)blockIdx.y * ROW_THREADS + threadIdx.x; i < size; i += (unsigned long long)PACK_PARTS * ROW_THREADS)
    packed[off + i] = s[i];
  if ((size & 1ull) && blockIdx.y == 0 && threadIdx.x == 0) packed[off + size] = 0;
}

}  // namespace

void launch_tiff_blocks(const TiffEncodeLaunch& a, hipStream_t s) {
  const long groups = (long)a.n_blocks * a.block_h;
  if (groups <= 0) return;
  DBM_CHECK(groups < (1L << 31), "dbm_tiff_encode: more than 2^31 block rows in one call");
  hipLaunchKernelGGL(tiff_blocks_kernel, dim3((unsigned)groups), dim3(ROW_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_tiff_lzw_encode(const TiffEncodeLaunch& a, hipStream_t s) {
  if (a.n_blocks <= 0) return;
  hipLaunchKernelGGL(tiff_lzw_encode_kernel, dim3((unsigned)a.n_blocks), dim3(64), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_tiff_pack(const uint8_t* src, size_t src_stride, const unsigned long long* table, int n_blocks, uint8_t* packed, hipStream_t s) {
  if (n_blocks <= 0) return;
  hipLaunchKernelGGL(tiff_pack_kernel, dim3((unsigned)n_blocks, PACK_PARTS), dim3(ROW_THREADS), 0, s, src, src_stride, table, packed);
  DBM_HIP(hipGetLastError());
}

size_t tiff_lzw_encode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) {
  std::vector<uint32_t> table(LZW_SLOTS);
  return lzw_encode_lanes(src, n, dst, cap, table.data(), 0u, 1u);
}
