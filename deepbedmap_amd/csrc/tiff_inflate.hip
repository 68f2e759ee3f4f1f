// Inflating the deflate blocks (Compression 8 / 32946) of a GeoTIFF on the device: stage (a') of dbm_tiff_decode, the
// twin of tiff_lzw_kernel in tiff_decode.hip.  Block b's zlib stream is decoded into stage + b * block_stride, where tiff_rows_kernel
// (predictors, conversion, placement) expects it whatever the codec was.
//
// Dialect: RFC 1950 around RFC 1951, accepted and refused as zlib's `uncompress` does it.  Header: CM = 8, CINFO <= 7, (CMF * 256 + FLG)
// % 31 == 0, no preset dictionary.  Stored blocks (byte alignment, LEN / NLEN), the fixed code, dynamic codes (HLIT / HDIST / HCLEN,
// the code-length alphabet in its permuted order, repeat codes 16 / 17 / 18 running across the literal -> distance boundary).  Refused:
// BTYPE 3, HLIT > 286 or HDIST > 30, a repeat with no previous length or past the last length, no end-of-block code, over-subscribed
// sets, incomplete sets (but one code of length 1, and no distance code at all, as zlib accepts them: using the missing code is the
// error), symbols 286 / 287, distance codes 30 / 31, a distance beyond what has been written, more output than the block holds, a
// stream that ends early, an Adler-32 that does not match the decoded bytes.  Bytes after the trailer are ignored.
//
// ONE WAVEFRONT PER BLOCK, as the LZW stage: inflate_lanes is parsed by all 64 lanes alike (every value that steers a loop is
// wave-uniform; on the device the values that come out of LDS are made scalar with readfirstlane), the lanes share the copies.
//   - the stream: 512 bytes of it lie in LDS (win), filled by one coalesced load per 64 bytes and read a 32-bit word at a time into a
//     64-bit bit buffer in registers (one word is read ahead).  The per-symbol loop touches registers and LDS only; global memory is
//     read once per 512 stream bytes, by the copy of a match farther back than the ring below holds, and by a stored block's copy.
//   - the codes: per deflate block the wave builds, in LDS, the canonical description of each code (cnt: codes per length; sym: the
//     symbols sorted by length, then value) and a first-level table indexed by the next 9 (literal/length) or 6 (distance, code-length
//     alphabet) bits, entry = symbol << 4 | length, 0 = "longer than that, or no code": each lane decodes its own table indices
//     canonically.  Longer codes are decoded canonically (at most 15 steps): lane l < 16 keeps cnt[l] in a register, the search for
//     the length reads those across the lanes, and one LDS read fetches the symbol.
//   - literals are collected one per lane and stored up to 64 at a time; a match is copied by the lanes, dst[outn + i] =
//     dst[outn - dist + i % dist].  The newest 4 096 output bytes are kept in LDS as well (ring[k % 4096] = byte k): a match of
//     distance <= 4096 - 258 reads its source there, so its stores wait for LDS only; a farther one reads the output in global memory
//     (what it needs was stored at least 3 838 bytes ago).  The Adler-32 is summed by the lanes afterwards (two 64-bit sums per lane,
//     reduced mod 65521).
// LDS per wave: sizeof(InflateTables) = 6 932 bytes (window 512, first-level tables 1 024 + 128, sorted symbols 576 + 64, counts and
// offsets 192, code lengths 320 + 20, ring 4 096), against the LZW stage's 32 KiB: 23 waves' worth fit a CU's 160 KiB, more than the
// 20 that the kernel's registers let a CU hold, so LDS does not limit the blocks resident per CU.
//
// Bounds and termination, by construction:
//   - the stream is read at byte indices < n only: the window's fill writes 0 for indices >= n, a stored block's copy is preceded by
//     p + LEN <= n.  The bit reader counts what it has consumed (8 * pos - have bits); after the header, every block header, every
//     code length, every symbol and the trailer, more than 8 * n consumed bits end the decoding as malformed, so the zeros are never
//     taken for data;
//   - every store to dst is preceded by outn (+ pending literals) + len <= cap;
//   - every copy source lies in [0, outn): dist <= outn is checked, the source index is outn - dist + (i % dist) < outn; ring indices
//     are masked to the ring's size, and the ring holds bytes [outn - 4096, outn) when a copy starts, of which the copy's own writes
//     replace [outn - 4096, outn + len - 4096): below outn - dist for dist <= 4096 - 258, so never a byte the copy still reads;
//   - table indices: the first-level index is masked to the table's size; a canonical decode indexes sym at index + code - first with
//     code - first < cnt[len], so below the number of symbols counted, which is at most the table's size (288 / 32) because nsym is; the
//     code lengths are written at idx + rep <= HLIT + HDIST <= 316 < 320 only; an over-subscribed set is refused before any decode;
//   - every iteration of every loop consumes at least one bit of the stream (a symbol's code is at least one bit long) or ends the
//     decoding; a copy runs over len <= cap bytes; a stored block's LEN is checked against the bytes left.
// Nothing is retried, nothing spins; a malformed stream ends in a status word.
// inflate_lanes is __host__ __device__: with (lane, lanes) = (0, 1) it is the host twin (dbm_inflate) that tools/inflate_twin_check.cpp
// runs against zlib and tests/test_inflate_host.py against zlib and a plain restatement.
#include "model.h"
#include "data_prims.h"

namespace {

// a value that is the same in every lane, as a scalar
__host__ __device__ inline uint32_t uni(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}

// arr[k], k wave-uniform and below 16, where every lane l < 16 holds arr[l] in `mine`: a cross-lane register read instead of LDS
__host__ __device__ inline uint32_t lane_get(uint32_t mine, uint32_t k, const uint32_t* arr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)k);
#else
  return arr[k];
#endif
}

__host__ __device__ inline void lanes_count(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, 1u);
#else
  ++*p;
#endif
}

constexpr uint32_t WIN = 512;          // bytes of the stream in LDS
constexpr uint32_t LIT_BITS = 9, DIST_BITS = 6;
constexpr uint32_t RING = 4096;        // bytes of the newest output kept in LDS as well: the source of matches up to RING - 258 back

struct InflateTables {
  uint32_t win[WIN / 4];               // the stream's bytes [wstart, wstart + 512), zeros past n; afterwards the lanes' Adler sums
  uint16_t lut_l[1 << LIT_BITS];       // symbol << 4 | code length, 0: not a code of <= 9 bits
  uint16_t lut_d[1 << DIST_BITS];      // (the code-length alphabet's while a dynamic header is read)
  uint16_t sym_l[288], sym_d[32];      // symbols sorted by code length, then value
  uint32_t cnt_l[16], cnt_d[16];       // codes per length
  uint32_t offs[16];                   // (sorting: where the next symbol of a length goes)
  uint8_t lens[320];                   // code lengths: literal/length symbols, then distance symbols
  uint8_t clens[20];                   // the code-length alphabet's lengths
  uint8_t ring[RING];                  // output byte k, for the newest RING of them, at ring[k % RING]
};

// The canonical decode of the low bits of `bits` (first bit of the code = bit 0): symbol << 4 | length, 0 if no code of <= maxlen bits
// matches.  U: `bits` is wave-uniform (the symbol loop) and lane l < 16 holds cnt[l] in `mine`, so the search for the length stays in
// registers and one LDS read fetches the symbol; otherwise per lane, counts from LDS (filling the first-level table).
template <bool U>
__host__ __device__ inline uint32_t canon(uint32_t bits, uint32_t maxlen, const uint32_t* cnt, const uint16_t* sym, uint32_t mine = 0) {
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= maxlen; ++len) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t c = U ? lane_get(mine, len, cnt) : cnt[len];
    if (code < first + c) {
      const uint32_t s = sym[index + (code - first)];
      return (U ? uni(s) : s) << 4 | len;
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

// Builds cnt / sym / lut of the code whose lengths are lens[0, nsym).  Returns 0, or 1 over-subscribed, or 2 incomplete; *max_len = the
// longest code (0: no code at all).
__host__ __device__ inline int build_code(const uint8_t* lens, uint32_t nsym, uint32_t* cnt, uint16_t* sym, uint32_t* offs, uint16_t* lut,
                                          uint32_t lutbits, uint32_t* max_len, uint32_t lane, uint32_t lanes) {
  for (uint32_t i = lane; i < 16; i += lanes) cnt[i] = 0;
  lanes_fence();
  for (uint32_t s = lane; s < nsym; s += lanes) lanes_count(&cnt[lens[s] & 15u]);
  lanes_fence();
  int left = 1;
  uint32_t run = 0, maxl = 0;
  bool over = false;
  for (uint32_t len = 1; len < 16; ++len) {
    const uint32_t c = uni(cnt[len]);
    left = 2 * left - (int)c;
    if (left < 0) { over = true; break; }   // (left <= 2^15 before: no overflow)
    if (c) maxl = len;
    if (lane == 0) offs[len] = run;
    run += c;
  }
  *max_len = maxl;
  if (over) return 1;
  lanes_fence();
  if (lane == 0)   // the symbols of one length keep their order: one lane
    for (uint32_t s = 0; s < nsym; ++s) {
      const uint32_t l = lens[s] & 15u;
      if (l) sym[offs[l]++] = (uint16_t)s;    // offs[l] < run <= nsym
    }
  lanes_fence();
  for (uint32_t i = lane; i < (1u << lutbits); i += lanes) lut[i] = (uint16_t)canon<false>(i, lutbits, cnt, sym);
  lanes_fence();
  return left > 0 ? 2 : 0;
}

// Decodes the zlib stream src[0, n) into dst[0, cap).  Returns the decoded size, or (size_t)-1 on everything the file header lists as
// refused.  All lanes of the wave call it with the same arguments but `lane`.
__host__ __device__ inline size_t inflate_lanes(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, InflateTables* t, uint32_t lane,
                                                uint32_t lanes) {
  constexpr size_t BAD = (size_t)-1;
  uint8_t* winb = (uint8_t*)t->win;
  size_t wstart = 0, outn = 0;
  uint32_t wpos = 0;         // byte index in the window of the next word for the bit buffer (a multiple of 4, < WIN)
  uint64_t acc = 0;          // the low `have` bits are the stream's next bits, first bit lowest
  uint32_t have = 0;
  uint32_t npend = 0;        // literals not stored yet: lane k holds the k-th in mylit
  uint8_t mylit = 0;
  bool fixed_built = false;
  uint32_t cl = 0, cd = 0;   // lane l < 16: cnt_l[l], cnt_d[l] of the codes in force (lane_get)

  // the bit reader.  NEED: afterwards have >= 33.  pos() = stream index of the next byte that goes into acc.
#define INF_FILL()                                                                              \
  do {                                                                                          \
    lanes_fence();                                                                              \
    for (uint32_t b_ = 0; b_ < WIN; b_ += 8 * lanes) { /* eight loads in flight (indices clamped to n - 1), then the stores */ \
      uint8_t v_[8];                                                                            \
      for (uint32_t k_ = 0; k_ < 8; ++k_) {                                                     \
        const size_t at_ = wstart + b_ + lane + k_ * lanes;                                     \
        v_[k_] = n ? src[at_ < n ? at_ : n - 1] : (uint8_t)0;                                   \
        if (at_ >= n) v_[k_] = 0;                                                               \
      }                                                                                         \
      for (uint32_t k_ = 0; k_ < 8; ++k_) winb[b_ + lane + k_ * lanes] = v_[k_];                \
    }                                                                                           \
    lanes_fence();                                                                              \
  } while (0)
#define INF_NEED()                                                                              \
  do {                                                                                          \
    if (have <= 32) {                                                                           \
      acc |= (uint64_t)uni(ahead) << have;                                                      \
      have += 32;                                                                               \
      wpos += 4;                                                                                \
      if (wpos == WIN) { wstart += WIN; wpos = 0; INF_FILL(); }                                 \
      ahead = t->win[wpos >> 2]; /* read now, awaited when it is needed */                      \
    }                                                                                           \
  } while (0)
#define INF_TAKE(var, nbits)                                                                    \
  do {                                                                                          \
    (var) = (uint32_t)acc & ((1u << (nbits)) - 1u);                                             \
    acc >>= (nbits);                                                                            \
    have -= (nbits);                                                                            \
  } while (0)
#define INF_OVERRUN() (8 * (uint64_t)(wstart + wpos) - have > 8 * (uint64_t)n)
#define INF_FLUSH()                                                                             \
  do {                                                                                          \
    if (npend) {                                                                                \
      if (lane < npend) {                                                                       \
        dst[outn + lane] = mylit;                                                               \
        t->ring[((uint32_t)outn + lane) & (RING - 1u)] = mylit;                                 \
      }                                                                                         \
      outn += npend;                                                                            \
      npend = 0;                                                                                \
    }                                                                                           \
  } while (0)

  INF_FILL();
  uint32_t ahead = t->win[0];   // the window's word at wpos, every lane its copy
  INF_NEED();
  uint32_t cmf, flg;
  INF_TAKE(cmf, 8);
  INF_TAKE(flg, 8);
  if (INF_OVERRUN()) return BAD;
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) + flg) % 31u != 0u || (flg & 0x20u)) return BAD;

  for (uint32_t last = 0; !last;) {
    INF_NEED();
    uint32_t btype;
    INF_TAKE(last, 1);
    INF_TAKE(btype, 2);
    if (INF_OVERRUN() || btype == 3) return BAD;
    if (btype == 0) {
      uint32_t drop, len, nlen;
      INF_TAKE(drop, have & 7u);   // to the byte boundary (whole words went into acc: `have` counts from it)
      (void)drop;
      INF_NEED();
      INF_TAKE(len, 16);
      INF_TAKE(nlen, 16);
      if (INF_OVERRUN() || (len ^ 0xFFFFu) != nlen) return BAD;
      const size_t p = wstart + wpos - have / 8;   // (<= n: no overrun)
      if (len > n - p) return BAD;
      INF_FLUSH();
      if (len > cap - outn) return BAD;
      for (uint32_t i = lane; i < len; i += lanes) {
        const uint8_t v = src[p + i];
        dst[outn + i] = v;
        t->ring[((uint32_t)outn + i) & (RING - 1u)] = v;   // (a pass writes 64 different places; later passes win)
      }
      outn += len;
      lanes_fence();
      // the reader starts over behind the copied bytes
      wstart = p + len; wpos = 0; acc = 0; have = 0;
      INF_FILL();
      ahead = t->win[0];
      continue;
    }
    if (btype == 1) {
      if (!fixed_built) {
        for (uint32_t s = lane; s < 320; s += lanes) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        lanes_fence();
        uint32_t m;
        build_code(t->lens, 288, t->cnt_l, t->sym_l, t->offs, t->lut_l, LIT_BITS, &m, lane, lanes);
        build_code(t->lens + 288, 32, t->cnt_d, t->sym_d, t->offs, t->lut_d, DIST_BITS, &m, lane, lanes);
        fixed_built = true;
      }
    } else {
      fixed_built = false;
      uint32_t nl, nd, nc, m;
      INF_TAKE(nl, 5);
      INF_TAKE(nd, 5);
      INF_TAKE(nc, 4);
      nl += 257; nd += 1; nc += 4;
      if (INF_OVERRUN() || nl > 286 || nd > 30) return BAD;
      // the code-length alphabet's lengths arrive in this order: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15 (5 bits each)
      const uint64_t order_a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                               5ull << 45 | 11ull << 50 | 4ull << 55;
      const uint64_t order_b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
      for (uint32_t i = lane; i < 20; i += lanes) t->clens[i] = 0;
      lanes_fence();
      for (uint32_t i = 0; i < nc; ++i) {
        uint32_t v;
        INF_NEED();
        INF_TAKE(v, 3);
        const uint32_t at = (uint32_t)((i < 12 ? order_a >> (5 * i) : order_b >> (5 * (i - 12))) & 31u);
        if (lane == 0) t->clens[at] = (uint8_t)v;
      }
      if (INF_OVERRUN()) return BAD;
      lanes_fence();
      // (zlib lets a code-length alphabet without any code through and fails on the end-of-block length 0 it then reads: refused here)
      if (build_code(t->clens, 19, t->cnt_d, t->sym_d, t->offs, t->lut_d, DIST_BITS, &m, lane, lanes) != 0 || m == 0) return BAD;
      cd = t->cnt_d[lane & 15u];
      const uint32_t total = nl + nd;   // <= 316
      uint32_t idx = 0, prev = 0;
      while (idx < total) {
        INF_NEED();
        uint32_t e = uni(t->lut_d[(uint32_t)acc & ((1u << DIST_BITS) - 1u)]);
        if (!e) e = canon<true>((uint32_t)acc, 7, t->cnt_d, t->sym_d, cd);
        if (!e) return BAD;
        uint32_t skip, s = e >> 4, rep = 1, val = s, x;
        INF_TAKE(skip, e & 15u);
        (void)skip;
        if (s == 16) {
          if (idx == 0) return BAD;
          INF_TAKE(x, 2);
          rep = 3 + x; val = prev;
        } else if (s == 17) {
          INF_TAKE(x, 3);
          rep = 3 + x; val = 0;
        } else if (s == 18) {
          INF_TAKE(x, 7);
          rep = 11 + x; val = 0;
        }
        if (INF_OVERRUN() || idx + rep > total) return BAD;
        for (uint32_t i = lane; i < rep; i += lanes) t->lens[idx + i] = (uint8_t)val;
        idx += rep;
        prev = val;
      }
      lanes_fence();
      if (uni(t->lens[256]) == 0) return BAD;   // no end-of-block code
      int rc = build_code(t->lens, nl, t->cnt_l, t->sym_l, t->offs, t->lut_l, LIT_BITS, &m, lane, lanes);
      if (rc == 1 || (rc == 2 && m != 1)) return BAD;
      rc = build_code(t->lens + nl, nd, t->cnt_d, t->sym_d, t->offs, t->lut_d, DIST_BITS, &m, lane, lanes);
      if (rc == 1 || (rc == 2 && m > 1)) return BAD;
    }
    cl = t->cnt_l[lane & 15u];
    cd = t->cnt_d[lane & 15u];
    // the block's symbols
    for (;;) {
      INF_NEED();
      uint32_t e = uni(t->lut_l[(uint32_t)acc & ((1u << LIT_BITS) - 1u)]);
      if (!e) e = canon<true>((uint32_t)acc, 15, t->cnt_l, t->sym_l, cl);
      if (!e) return BAD;
      uint32_t skip, s = e >> 4;
      INF_TAKE(skip, e & 15u);
      (void)skip;
      if (s < 256) {
        if (INF_OVERRUN() || outn + npend >= cap) return BAD;
        if (lane == npend) mylit = (uint8_t)s;
        if (++npend == lanes) INF_FLUSH();
        continue;
      }
      if (s == 256) {
        if (INF_OVERRUN()) return BAD;
        break;
      }
      if (s >= 286) return BAD;
      uint32_t len = 258, dist, x;
      if (s < 285) {
        const uint32_t k = s - 257;
        if (k < 8) {
          len = 3 + k;
        } else {
          const uint32_t eb = (k >> 2) - 1;
          INF_TAKE(x, eb);
          len = 3 + ((4 + (k & 3u)) << eb) + x;
        }
      }
      INF_NEED();
      e = uni(t->lut_d[(uint32_t)acc & ((1u << DIST_BITS) - 1u)]);
      if (!e) e = canon<true>((uint32_t)acc, 15, t->cnt_d, t->sym_d, cd);
      if (!e) return BAD;
      const uint32_t d = e >> 4;
      INF_TAKE(skip, e & 15u);
      if (d >= 30) return BAD;
      if (d < 4) {
        dist = 1 + d;
      } else {
        const uint32_t eb = (d >> 1) - 1;
        INF_TAKE(x, eb);
        dist = 1 + ((2 + (d & 1u)) << eb) + x;
      }
      if (INF_OVERRUN()) return BAD;
      INF_FLUSH();
      if (dist > outn || len > cap - outn) return BAD;
      lanes_fence();
      // the source: the ring where it still holds it while this copy writes its own len <= 258 bytes there, else the output itself
      const bool near = dist <= RING - 258u;
      const uint32_t o = (uint32_t)outn;
      const uint8_t* from = dst + (outn - dist);
      if (near) {   // (two loops: one load from LDS, one from global memory, never a load that could be either)
        for (uint32_t i = lane; i < len; i += lanes) {
          const uint8_t v = t->ring[(o - dist + (dist >= len ? i : i % dist)) & (RING - 1u)];
          dst[outn + i] = v;
          t->ring[(o + i) & (RING - 1u)] = v;
        }
      } else {
        for (uint32_t i = lane; i < len; i += lanes) {
          const uint8_t v = from[dist >= len ? i : i % dist];
          dst[outn + i] = v;
          t->ring[(o + i) & (RING - 1u)] = v;
        }
      }
      outn += len;
      lanes_fence();
    }
  }
  INF_FLUSH();
  // the trailer: to the byte boundary, then the Adler-32 of the decoded bytes, most significant byte first
  uint32_t drop, lo, hi;
  INF_TAKE(drop, have & 7u);
  (void)drop;
  INF_NEED();
  INF_TAKE(lo, 16);
  INF_TAKE(hi, 16);
  if (INF_OVERRUN()) return BAD;
  const uint32_t stored = (lo & 0xFFu) << 24 | (lo >> 8) << 16 | (hi & 0xFFu) << 8 | (hi >> 8);
#undef INF_FILL
#undef INF_NEED
#undef INF_TAKE
#undef INF_OVERRUN
#undef INF_FLUSH
  // a = 1 + sum b[i], b = n + sum (n - i) b[i] (mod 65521): each lane sums the bytes i = lane (mod lanes); a term stays below 2^39, 4096
  // of them below 2^51
  lanes_fence();
  uint64_t s1 = 0, s2 = 0;
  uint32_t since = 0;
  for (size_t base = 0; base < outn; base += 8 * (size_t)lanes) {   // eight loads in flight (indices clamped to outn - 1)
    uint8_t v[8];
    for (uint32_t k = 0; k < 8; ++k) {
      const size_t i = base + lane + k * (size_t)lanes;
      v[k] = dst[i < outn ? i : outn - 1];
    }
    for (uint32_t k = 0; k < 8; ++k) {
      const size_t i = base + lane + k * (size_t)lanes;
      if (i < outn) {
        s1 += v[k];
        s2 += (uint64_t)(outn - i) * v[k];
      }
    }
    if (++since == 512) { s2 %= 65521u; since = 0; }
  }
  t->win[2 * (lane % 64u)] = (uint32_t)(s1 % 65521u);
  t->win[2 * (lane % 64u) + 1] = (uint32_t)(s2 % 65521u);
  lanes_fence();
  uint64_t a = 1, b = outn % 65521u;
  for (uint32_t k = 0; k < lanes; ++k) {
    a += uni(t->win[2 * k]);
    b += uni(t->win[2 * k + 1]);
  }
  if (((uint32_t)(b % 65521u) << 16 | (uint32_t)(a % 65521u)) != stored) return BAD;
  return outn;
}

__global__ __launch_bounds__(64) void tiff_inflate_kernel(StreamDecodeLaunch a) {
  __shared__ InflateTables t;
  const long b = blockIdx.x;
  const long* e = a.blocks + 8 * b;
  const size_t want = (size_t)(a.whole_rows ? a.whole_rows : e[2]) * (size_t)a.row_bytes;   // <= block_stride (checked by the caller)
  const size_t got = inflate_lanes(a.streams + e[0], (size_t)e[1], a.stage + b * a.block_stride, want, &t, threadIdx.x, 64u);
  if (threadIdx.x == 0) a.status[b] = got == (size_t)-1 ? 1 : (got != want ? 2 : 0);
}

}  // namespace

void launch_block_inflate(const StreamDecodeLaunch& a, hipStream_t s) {
  if (a.n_blocks <= 0) return;
  hipLaunchKernelGGL(tiff_inflate_kernel, dim3((unsigned)a.n_blocks), dim3(64), 0, s, a);
  DBM_HIP(hipGetLastError());
}

size_t tiff_inflate_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap) {
  InflateTables t;
  return inflate_lanes(src, n, dst, cap, &t, 0u, 1u);
}

extern "C" int dbm_inflate(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes) {
  if (!src || !dst || !out_bytes) return 1;
  const size_t n = tiff_inflate_twin((const uint8_t*)src, nbytes, (uint8_t*)dst, cap);
  if (n == (size_t)-1) return 2;
  *out_bytes = n;
  return 0;
}
