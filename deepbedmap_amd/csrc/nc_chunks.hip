// Placing the chunks of a netCDF variable on the device (dbm_chunk_decode; the host side -- the HDF5 / classic container, the chunk plan,
// reading the streams -- is deepbedmap_amd/netcdf.py).  Replaces the reference's xarray / rasterio reads of netCDF grids
// (data_prep.py:889-900, deepbedmap.py:74-78, :176-191).  DESIGN.md 6l.
//
// Deflated chunks are inflated by launch_block_inflate (tiff_inflate.hip, one wavefront per block) into the staging area, as for
// dbm_tiff_decode; uncompressed chunks and the row bands of contiguous / classic data are read where they were uploaded.  ONE kernel
// then does everything else, one pass over the staged bytes:
//   - HDF5's shuffle filter is undone while reading: with shuffle on, byte k (in memory order) of element i of the block lies at
//     k * n + i, n = block_h * block_w -- `bytes` loads from `bytes` byte planes, no un-shuffled copy of the block ever exists;
//   - the bytes are put in order for either endianness (big endian: memory byte 0 is the most significant);
//   - the sample is compared with the fill BY VALUE in its stored type (integers: the bits; floats: ==, so -0.0 equals 0.0, and a NaN
//     fill matches every NaN) -> NaN (0x7fc00000);
//   - otherwise float32(float64(v) * scale + offset) as two separately rounded float64 operations (nc_scale_offset: contraction into
//     an FMA is switched off there, NumPy rounds twice), or numpy.astype(float32) without a scale (float32 keeps its bits);
//   - the value is stored at output row e[3] + step * r, column e[4] + c; samples outside the plane are dropped.
//
// Mapping.  A workgroup does not own a block row: chunks are often narrow (32 x 16, 8 x 8), and a row of 16 samples would keep 16 of a
// wavefront's 64 lanes busy.  The block is taken as the flat run of its n elements instead: thread t of workgroup g handles elements
// (g * PASSES + p) * THREADS + t, p = 0 .. PASSES - 1, and derives (row, column) by one 32-bit division.  Adjacent lanes therefore
// always hold adjacent elements, whatever block_w is: each byte-plane load of a wavefront is 64 consecutive bytes (a whole-sample load
// 64 * bytes consecutive bytes), and the float stores are contiguous runs of min(block_w, 64) floats per output row -- a 16-wide chunk
// gives a wavefront four full rows of work, not a quarter of one.  Only the last workgroup of a block has idle lanes.  Nothing is shared
// between threads: no LDS, no barrier, no atomics.
#include "model.h"

namespace {

constexpr int NC_THREADS = 256;
constexpr int NC_PASSES = 4;

// the sample's bits, the memory bytes put in value order
__device__ inline unsigned long long nc_load(const uint8_t* src, unsigned i, unsigned n, int bytes, bool shuffle, bool big) {
  unsigned long long raw = 0;
  if (shuffle) {
    for (int k = 0; k < bytes; ++k) {
      const unsigned long long byte = src[(size_t)k * n + i];
      raw |= byte << (8 * (big ? bytes - 1 - k : k));
    }
    return raw;
  }
  switch (bytes) {   // (the block starts at a multiple of 8 bytes: every sample is aligned to its own width)
    case 1: return src[i];
    case 2: { const uint16_t v = ((const uint16_t*)src)[i]; return big ? (uint16_t)((v << 8) | (v >> 8)) : v; }
    case 4: { const uint32_t v = ((const uint32_t*)src)[i]; return big ? __builtin_bswap32(v) : v; }
    default: { const unsigned long long v = ((const unsigned long long*)src)[i]; return big ? __builtin_bswap64(v) : v; }
  }
}

// float64(v) * scale + offset as NumPy computes it: the product rounded, then the sum rounded.  Contraction is switched off for this
// function: HIP's __dmul_rn / __dadd_rn are plain `*` and `+` to the compiler, which fuses them into one v_fma_f64 under its default
// -ffp-contract=fast-honor-pragmas (tests/test_gpu_netcdf.py has the sample where the fused result differs).
__device__ inline double nc_scale_offset(double v, double scale, double offset) {
#pragma clang fp contract(off)
  const double product = v * scale;
  return product + offset;
}

__global__ __launch_bounds__(NC_THREADS) void nc_chunks_kernel(ChunkDecodeLaunch a) {
  const long b = (long)(blockIdx.x / a.groups_per_block);
  const unsigned g = blockIdx.x - (unsigned)b * a.groups_per_block;
  const long* e = a.blocks + 8 * b;
  const uint8_t* src = a.staged ? a.stage + b * a.block_stride : a.stage + e[0];
  const unsigned bw = (unsigned)a.block_w;
  const unsigned n = (unsigned)a.block_h * bw;       // < 2^31 (checked by the caller)
  const unsigned held = (unsigned)e[2] * bw;         // rows held <= block_h
  const long orow0 = e[3], ocol0 = e[4], step = e[6];
  const bool shuffle = a.shuffle != 0, big = a.big_endian != 0;
#pragma unroll
  for (int p = 0; p < NC_PASSES; ++p) {
    const unsigned i = (g * NC_PASSES + p) * NC_THREADS + threadIdx.x;
    if (i >= held) return;
    const unsigned r = i / bw, c = i - r * bw;
    const long orow = orow0 + step * (long)r, ocol = ocol0 + (long)c;
    if (orow < 0 || orow >= a.out_h || ocol < 0 || ocol >= a.out_w) continue;
    const unsigned long long raw = nc_load(src, i, n, a.bytes, shuffle, big);
    double d;          // the value, exact in float64 for every type
    uint32_t plain;    // numpy.astype(float32) of it
    bool masked;
    switch (a.sample_type) {
      case 0: { const uint8_t v = (uint8_t)raw; d = v; plain = __float_as_uint((float)v); masked = raw == a.fill_bits; break; }
      case 1: { const int16_t v = (int16_t)(uint16_t)raw; d = v; plain = __float_as_uint((float)v); masked = raw == a.fill_bits; break; }
      case 2: { const uint16_t v = (uint16_t)raw; d = v; plain = __float_as_uint((float)v); masked = raw == a.fill_bits; break; }
      case 3: { const int32_t v = (int32_t)(uint32_t)raw; d = v; plain = __float_as_uint((float)v); masked = raw == a.fill_bits; break; }
      case 4: {
        const float v = __uint_as_float((uint32_t)raw), f = __uint_as_float((uint32_t)a.fill_bits);
        d = (double)v; plain = (uint32_t)raw;                                   // float32: the bits, NaN payloads included
        masked = v == f || (v != v && f != f);
        break;
      }
      case 5: {
        const double v = __longlong_as_double((long long)raw), f = __longlong_as_double((long long)a.fill_bits);
        d = v; plain = __float_as_uint((float)v);
        masked = v == f || (v != v && f != f);
        break;
      }
      default: { const int8_t v = (int8_t)(uint8_t)raw; d = v; plain = __float_as_uint((float)v); masked = raw == a.fill_bits; break; }
    }
    uint32_t bits;
    if (a.has_fill && masked) bits = 0x7fc00000u;
    else if (a.has_scale) bits = __float_as_uint((float)nc_scale_offset(d, a.scale, a.offset));   // two roundings, then one: no FMA
    else bits = plain;
    ((uint32_t*)a.out)[orow * a.out_w + ocol] = bits;
  }
}

// The inverse (dbm_chunk_encode, stage (a)): chunk b of the call as the bytes an HDF5 file holds before deflate.  The same mapping as
// above: the chunk is the flat run of its n elements, thread t of workgroup g takes elements (g * PASSES + p) * THREADS + t, so a
// wavefront loads runs of min(chunk_w, 64) consecutive floats of a plane row and stores 64 consecutive bytes to each byte plane (64
// consecutive words without shuffle).  The values are loaded as integers: NaN payloads and -0.0 pass unchanged.
__global__ __launch_bounds__(NC_THREADS) void nc_chunk_cut_kernel(ChunkEncodeLaunch a) {
  const long b = (long)(blockIdx.x / a.groups_per_block);
  const unsigned g = blockIdx.x - (unsigned)b * a.groups_per_block;
  const long index = a.first + b, cy = index / a.chunks_x, cx = index - cy * a.chunks_x;
  const long r0 = cy * a.chunk_h, c0 = cx * a.chunk_w;
  const unsigned cw = (unsigned)a.chunk_w;
  const unsigned n = (unsigned)a.chunk_h * cw;       // n * 4 < 2^31 (checked by the caller)
  uint8_t* out = a.raw + b * a.raw_stride;
  const uint32_t* plane = (const uint32_t*)a.plane;
#pragma unroll
  for (int p = 0; p < NC_PASSES; ++p) {
    const unsigned i = (g * NC_PASSES + p) * NC_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned r = i / cw, c = i - r * cw;
    const long row = r0 + (long)r, col = c0 + (long)c;
    uint32_t bits = 0u;   // the padding of an edge chunk
    if (row < a.H && col < a.W) bits = plane[(a.row_step > 0 ? row : a.H - 1 - row) * a.W + col];
    if (a.shuffle) {
      for (int k = 0; k < 4; ++k) out[(size_t)k * n + i] = (uint8_t)(bits >> (8 * k));
    } else {
      ((uint32_t*)out)[i] = bits;   // (raw_stride is a multiple of 16: aligned)
    }
  }
}

}  // namespace

void launch_nc_chunk_cut(const ChunkEncodeLaunch& a, hipStream_t s) {
  const long groups = (long)a.n_blocks * a.groups_per_block;
  if (groups <= 0) return;
  DBM_CHECK(groups < (1L << 31), "dbm_chunk_encode: more than 2^31 workgroups in one call");
  hipLaunchKernelGGL(nc_chunk_cut_kernel, dim3((unsigned)groups), dim3(NC_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

unsigned nc_chunks_groups_per_block(int block_w, int block_h) {
  const long n = (long)block_w * block_h, per = (long)NC_THREADS * NC_PASSES;
  return (unsigned)((n + per - 1) / per);
}

void launch_nc_chunks(const ChunkDecodeLaunch& a, hipStream_t s) {
  const long groups = (long)a.n_blocks * a.groups_per_block;
  if (groups <= 0) return;
  DBM_CHECK(groups < (1L << 31), "dbm_chunk_decode: more than 2^31 workgroups in one call");
  hipLaunchKernelGGL(nc_chunks_kernel, dim3((unsigned)groups), dim3(NC_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}
