// Deflating blocks of bytes on the device (launch_block_deflate: the chunks of a netCDF-4 variable, dbm_chunk_encode) and on the host
// (dbm_deflate_encode_blocks).  The mirror of tiff_inflate.hip; DESIGN.md 6m has the rule statement by statement.
//
// Stream.  One zlib stream (RFC 1950 around RFC 1951) per block: the header 78 01, ONE final block with the fixed Huffman code
// (BFINAL 1, BTYPE 01), the Adler-32 of the input.  No dynamic codes, no stored blocks, never a second deflate block.
//
// Rule (this project's own; the stream is a function of the input bytes alone).  A table of 16 384 16-bit entries, all zero at the
// start.  hash(p) = ((b[p] | b[p+1] << 8 | b[p+2] << 16) * 2654435761 mod 2^32) >> 18, defined for p + 2 < n.  insert(p): table[hash(p)]
// = p mod 65536 -- positions are inserted in ascending order, so an entry always holds the LARGEST position inserted with its hash.
// At position i, while i < n:
//   1. if i + 3 <= n: s = table[hash(i)], dist = (i - s) mod 65536; the candidate i - dist is taken if 1 <= dist <= 32768 and
//      dist <= i (an entry is 16 bits: a position that is 65536 older reads alike, and the zeros of the start read as position 0 --
//      whatever a candidate is, only the bytes decide);
//   2. len = the number of equal bytes b[i - dist + k] == b[i + k], k < min(258, n - i);
//   3. len >= 3: the match (len, dist) is written and the positions i .. i + len - 1 are inserted (those with p + 2 < n); i += len.
//      Otherwise: the literal b[i] is written, i is inserted (if i + 2 < n); i += 1.
// Greedy: the first candidate is the only one, no lazy evaluation.
//
// ONE WAVEFRONT PER BLOCK, control wave-uniform; the lanes do the wide work: the Adler-32 (lane l sums the bytes l, l + 64, ... with
// their weights, one reduction at the end), the match length (64 bytes of both sides per step and a ballot), the inserts of a match's
// span (64 positions per step).  Two lanes of one step may hash to the same entry; the rule says the larger position stays.  There
// is no 16-bit LDS atomic, so: every lane stores, the wave reads back, and every lane that finds a LOWER lane's position stores again,
// until none does -- each repetition raises what the entry holds, so it ends after at most 63, and what it ends with is the largest
// lane's position whichever store the hardware kept in between: the entry's final value does not depend on that.  The table is
// 32 KiB of LDS: five waves per CU.
// Bounds, by construction: the input is read below n only (every load is guarded); every output store is preceded by `count < cap`
// -- on overflow the flag is set, the loop ends, 0 is returned (status word 1) and nothing is written at or past cap; every iteration
// of the main loop consumes at least one input byte; nothing is retried, nothing spins.  A literal costs at most 9 bits, a match at most
// 31 for at least 11 bytes or 25 for at least 3: never more than 9 bits per input byte, so n + n / 8 + 16 bytes (deflate_slot) always
// hold the stream.
// deflate_encode_lanes is __host__ __device__: with (lane, lanes) = (0, 1) it is the host encoder.  Only the lane primitives differ
// between the two compilations: window_byte, equal_run, insert_span and lanes_sum.
//
// Framing (the bands of a PNG are segments of ONE zlib stream that the host stitches).  The rule above -- hash, candidate,
// match, inserts -- is the same in every mode; a segment starts with an empty table, so it never refers to bytes in front of it.
//   0  the stream described above: 78 01, BFINAL 1, the Adler-32 behind the block.
//   1  a middle segment: no header; one block BFINAL 0, BTYPE 01; behind its end-of-block symbol an EMPTY STORED block -- the bits 000
//      (BFINAL 0, BTYPE 00), zero bits up to the next byte boundary, then LEN 00 00 and NLEN FF FF -- so that the segment ends on a
//      byte boundary and the next one can be appended (what zlib's Z_SYNC_FLUSH writes).  No Adler-32 in the stream.
//   2  the last segment: no header; BFINAL 1; end-of-block; zero bits up to the byte boundary.  No Adler-32 in the stream.
// In modes 1 and 2 the Adler-32 of the segment's input goes to *adler_out (the caller joins the segments' sums: adler32_combine).
// The slot bound holds in every mode: the symbols cost at most 9 n bits; mode 0 adds 2 + 4 bytes and 3 + 7 bits, mode 1 adds 3 + 7 + 3
// bits, at most 7 bits of padding and 4 bytes, mode 2 adds 3 + 7 bits and the padding: never more than ceil((9 n + 20) / 8) + 6 <=
// n + n / 8 + 10 bytes, below n + n / 8 + 16.
#include "model.h"
#include "data_prims.h"
#include <thread>

namespace {

constexpr uint32_t DEFLATE_HASH_BITS = 14, DEFLATE_SLOTS = 1u << DEFLATE_HASH_BITS;
constexpr uint32_t DEFLATE_WINDOW = 32768, DEFLATE_MAX_MATCH = 258, DEFLATE_MIN_MATCH = 3;
constexpr uint32_t ADLER_MOD = 65521;

__host__ __device__ inline uint32_t deflate_hash(uint32_t b0, uint32_t b1, uint32_t b2) {
  return ((b0 | (b1 << 8) | (b2 << 16)) * 2654435761u) >> (32 - DEFLATE_HASH_BITS);
}

// ---- lane primitives: the only code that differs between the device and the host encoder ----
// Input byte i + k (k < 3, i + k < n).  Device: lane l holds src[i + l] in `mine`.
__host__ __device__ inline uint32_t window_byte(const uint8_t* src, size_t i, uint32_t k, uint32_t mine) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)src; (void)i;
  return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)k);
#else
  (void)mine;
  return src[i + k];
#endif
}

// The number of leading k < count (<= 64) with src[a + k] == src[b + k]; the caller keeps a + count and b + count within n.
__host__ __device__ inline uint32_t equal_run(const uint8_t* src, size_t a, size_t b, uint32_t count, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  const bool differs = lane >= count || src[a + lane] != src[b + lane];
  const unsigned long long mask = __ballot(differs);
  return mask ? (uint32_t)__builtin_ctzll(mask) : 64u;   // (count <= 64: a lane at or past count stops the run)
#else
  (void)lane;
  uint32_t k = 0;
  while (k < count && src[a + k] == src[b + k]) ++k;
  return k;
#endif
}

// insert(p) for p = p0 .. p0 + count - 1 (count <= 64) where p + 2 < n: afterwards every entry touched holds its largest such p.
__host__ __device__ inline void insert_span(uint16_t* table, const uint8_t* src, size_t n, size_t p0, uint32_t count, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  const size_t p = p0 + lane;
  const bool act = lane < count && p + 2 < n;
  const uint32_t h = act ? deflate_hash(src[p], src[p + 1], src[p + 2]) : 0u;
  const uint16_t mine = (uint16_t)p, first = (uint16_t)p0;
  if (act) table[h] = mine;
  lanes_fence();
#pragma unroll 1
  for (int round = 0; round < 64; ++round) {
    // what the entry holds is a position of this step: its distance from p0 is the lane that stored it
    const bool again = act && (uint32_t)(uint16_t)(table[h] - first) < lane;
    if (!__ballot(again)) break;
    if (again) table[h] = mine;
    lanes_fence();
  }
#else
  (void)lane;
  for (uint32_t k = 0; k < count; ++k) {
    const size_t p = p0 + k;
    if (p + 2 < n) table[deflate_hash(src[p], src[p + 1], src[p + 2])] = (uint16_t)p;
  }
#endif
}

// the sum of v over the lanes, in every lane (host: v)
__host__ __device__ inline unsigned long long lanes_sum(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int off = 32; off > 0; off >>= 1) v += wave_words(v, [off](int w) { return __shfl_xor(w, off, 64); });
#endif
  return v;
}

// LSB-first bit packer of RFC 1951; lane 0 stores.  A byte is stored only while count < cap.
struct DeflateBitWriter {
  uint8_t* out;
  size_t cap, count;
  unsigned long long acc;
  uint32_t bits, lane;
  bool overflow;
  __host__ __device__ inline void emit(uint32_t byte) {
    if (count < cap) {
      if (lane == 0) out[count] = (uint8_t)byte;
    } else {
      overflow = true;
    }
    ++count;
  }
  // bits <= 7 before and width <= 31: at most 38 bits in use, at most four whole bytes leave
  __host__ __device__ inline void put(uint32_t value, uint32_t width) {
    acc |= (unsigned long long)value << bits;
    bits += width;
    while (bits >= 8) {
      emit((uint32_t)(acc & 0xFFu));
      acc >>= 8;
      bits -= 8;
    }
  }
  // a Huffman code goes most significant bit first
  __host__ __device__ inline void put_code(uint32_t code, uint32_t width) { put(__builtin_bitreverse32(code) >> (32 - width), width); }
  __host__ __device__ inline void flush() {
    if (bits > 0) {
      emit((uint32_t)(acc & 0xFFu));
      acc = 0;
      bits = 0;
    }
  }
};

__host__ __device__ inline uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// literal / length symbol of the fixed code (RFC 1951 3.2.6)
__host__ __device__ inline void put_symbol(DeflateBitWriter& w, uint32_t sym) {
  if (sym < 144u) w.put_code(0x30u + sym, 8);
  else if (sym < 256u) w.put_code(0x190u + (sym - 144u), 9);
  else if (sym < 280u) w.put_code(sym - 256u, 7);
  else w.put_code(0xC0u + (sym - 280u), 8);
}

// a match of len 3..258 at dist 1..32768 (RFC 1951 3.2.5: the symbol, its extra bits, the 5-bit distance code, its extra bits)
__host__ __device__ inline void put_match(DeflateBitWriter& w, uint32_t len, uint32_t dist) {
  const uint32_t l = len - 3u;
  if (len == 258u) {
    put_symbol(w, 285u);
  } else if (l < 8u) {
    put_symbol(w, 257u + l);
  } else {
    const uint32_t e = floor_log2(l) - 2u;   // 1..5 extra bits
    put_symbol(w, 257u + 4u * e + (l >> e));
    w.put(l & ((1u << e) - 1u), e);
  }
  const uint32_t d = dist - 1u;
  if (d < 4u) {
    w.put_code(d, 5);
  } else {
    const uint32_t e = floor_log2(d) - 1u;   // 1..13 extra bits
    w.put_code(2u * (e + 1u) + ((d >> e) & 1u), 5);   // the bit below the leading one picks the code of the pair
    w.put(d & ((1u << e) - 1u), e);
  }
}

// Adler-32 of src[0, n): a = 1 + sum b[k], b = n + sum (n - k) b[k], both mod 65521; lane l takes k = l, l + lanes, ...
__host__ __device__ inline uint32_t adler32_lanes(const uint8_t* src, size_t n, uint32_t lane, uint32_t lanes) {
  unsigned long long s1 = 0, s2 = 0;
  uint32_t weight = (uint32_t)((n - (lane < n ? lane : n)) % ADLER_MOD);   // (n - k) mod 65521, kept by subtracting `lanes` each step
  uint32_t steps = 0;
  for (size_t k = lane; k < n; k += lanes) {
    const uint32_t b = src[k];
    s1 += b;
    s2 += (unsigned long long)weight * b;
    weight = weight >= lanes ? weight - lanes : weight + ADLER_MOD - lanes;
    if (++steps == (1u << 20)) {   // (s2 grows by less than 2^24 a step: reduced long before 2^64)
      s1 %= ADLER_MOD;
      s2 %= ADLER_MOD;
      steps = 0;
    }
  }
  s1 = lanes_sum(s1 % ADLER_MOD);
  s2 = lanes_sum(s2 % ADLER_MOD);
  const uint32_t a = (uint32_t)((1ull + s1) % ADLER_MOD), b = (uint32_t)((n % ADLER_MOD + s2) % ADLER_MOD);
  return (b << 16) | a;
}

// Encodes src[0, n) into dst[0, cap).  Returns the encoded size, or 0 if cap is too small.  table: DEFLATE_SLOTS entries,
// uninitialised.  All lanes of the wave call it with the same arguments but `lane`.
// framing: 0 a whole zlib stream, 1 a middle segment, 2 the last segment (the head of this file); adler_out: where modes 1 and 2 leave
// the Adler-32 of src[0, n) (lane 0 stores; may be null in mode 0).
__host__ __device__ inline size_t deflate_encode_lanes(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, uint16_t* table, uint32_t lane,
                                                       uint32_t lanes, uint32_t framing = 0u, uint32_t* adler_out = nullptr) {
  DeflateBitWriter w{dst, cap, 0, 0ull, 0u, lane, false};
  for (uint32_t k = lane; k < DEFLATE_SLOTS; k += lanes) table[k] = 0;
  lanes_fence();
  const uint32_t adler = adler32_lanes(src, n, lane, lanes);
  if (framing == 0u) {
    w.emit(0x78u);
    w.emit(0x01u);
  }
  w.put(framing == 1u ? 0u : 1u, 1);   // BFINAL
  w.put(1u, 2);                        // BTYPE 01: the fixed code
  size_t i = 0;
#pragma unroll 1
  while (i < n && !w.overflow) {
    const uint32_t mine = i + lane < n ? src[i + lane] : 0u;   // the next 64 bytes, one per lane (host: unused)
    const uint32_t b0 = window_byte(src, i, 0, mine);
    uint32_t len = 0, dist = 0;
    if (i + DEFLATE_MIN_MATCH <= n) {
      const uint32_t h = deflate_hash(b0, window_byte(src, i, 1, mine), window_byte(src, i, 2, mine));
      dist = ((uint32_t)i - (uint32_t)table[h]) & 0xFFFFu;
      if (dist >= 1u && dist <= DEFLATE_WINDOW && dist <= i) {
        const size_t left = n - i;
        const uint32_t most = left < DEFLATE_MAX_MATCH ? (uint32_t)left : DEFLATE_MAX_MATCH;
#pragma unroll 1
        while (len < most) {
          const uint32_t count = most - len < 64u ? most - len : 64u;
          const uint32_t run = equal_run(src, i - dist + len, i + len, count, lane);
          len += run;
          if (run < count) break;
        }
      }
    }
    if (len >= DEFLATE_MIN_MATCH) {
      put_match(w, len, dist);
#pragma unroll 1
      for (uint32_t k = 0; k < len; k += 64u) insert_span(table, src, n, i + k, len - k < 64u ? len - k : 64u, lane);
      i += len;
    } else {
      put_symbol(w, b0);
      if (i + 2 < n) {
        if (lane == 0) table[deflate_hash(b0, window_byte(src, i, 1, mine), window_byte(src, i, 2, mine))] = (uint16_t)i;
        lanes_fence();
      }
      i += 1;
    }
  }
  if (w.overflow) return 0;
  put_symbol(w, 256u);   // end of block
  if (framing == 1u) w.put(0u, 3);   // the empty stored block: BFINAL 0, BTYPE 00
  w.flush();
  if (framing == 0u) {
    w.emit(adler >> 24);
    w.emit((adler >> 16) & 0xFFu);
    w.emit((adler >> 8) & 0xFFu);
    w.emit(adler & 0xFFu);
  } else {
    if (framing == 1u) {   // LEN 0, NLEN ~0
      w.emit(0x00u);
      w.emit(0x00u);
      w.emit(0xFFu);
      w.emit(0xFFu);
    }
    if (lane == 0 && adler_out) *adler_out = adler;
  }
  return w.overflow ? 0 : w.count;
}

__global__ __launch_bounds__(64) void block_deflate_kernel(DeflateLaunch a) {
  __shared__ uint16_t table[DEFLATE_SLOTS];
  const size_t b = blockIdx.x;
  // segments (a.segments: the bands of a PNG): every block is a middle segment but the one that ends the stream, which may be short
  const bool last = a.segments && (long)b == a.last_block;
  const size_t n = last ? a.last_bytes : a.block_bytes;
  const uint32_t framing = a.segments ? (last ? 2u : 1u) : 0u;
  const size_t got = deflate_encode_lanes(a.raw + b * a.raw_stride, n, a.slots + b * a.slot_cap, a.slot_cap, table, threadIdx.x, 64u, framing,
                                          a.segments ? a.segment_words + 2 * b : nullptr);
  if (threadIdx.x == 0) {
    a.result[2 * b] = (uint32_t)got;             // (slot_cap < 2^32: block_bytes < 2^31)
    a.result[2 * b + 1] = got == 0 ? 1u : 0u;    // the status word: 1 = the stream did not fit its slot
    if (a.segments) a.segment_words[2 * b + 1] = (uint32_t)n;   // (behind the segment's Adler-32: its length)
  }
}

}  // namespace

void launch_block_deflate(const DeflateLaunch& a, hipStream_t s) {
  if (a.n_blocks <= 0) return;
  hipLaunchKernelGGL(block_deflate_kernel, dim3((unsigned)a.n_blocks), dim3(64), 0, s, a);
  DBM_HIP(hipGetLastError());
}

size_t deflate_encode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, uint16_t* table, int framing, uint32_t* adler_out) {
  return deflate_encode_lanes(src, n, dst, cap, table, 0u, 1u, (uint32_t)framing, adler_out);
}

extern "C" int dbm_deflate_encode_blocks(const void* blocks, size_t block_bytes, int nblocks, void* out, size_t out_stride, size_t* out_sizes,
                                         int nthreads) {
  if (!blocks || !out || !out_sizes || nblocks < 0) return 1;
  if (nthreads < 1) nthreads = 1;
  if (nthreads > nblocks) nthreads = nblocks > 0 ? nblocks : 1;
  auto work = [&](int t0) {
    std::vector<uint16_t> table(DEFLATE_SLOTS);
    for (int t = t0; t < nblocks; t += nthreads)
      out_sizes[t] = deflate_encode_lanes((const uint8_t*)blocks + (size_t)t * block_bytes, block_bytes, (uint8_t*)out + (size_t)t * out_stride,
                                          out_stride, table.data(), 0u, 1u);
  };
  std::vector<std::thread> th;
  for (int i = 1; i < nthreads; ++i) th.emplace_back(work, i);
  work(0);
  for (auto& t : th) t.join();
  for (int t = 0; t < nblocks; ++t)
    if (out_sizes[t] == 0) return 2;   // out_stride too small (block_bytes + block_bytes / 8 + 16 is always enough)
  return 0;
}
