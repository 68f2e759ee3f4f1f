// Survey text tables -> float64 tables (reference data_prep.py:298-305: `pandas.read_csv(f, sep, header=skip, names, usecols, na_values)`
// followed by `dropna`).  The dialect is defined in DESIGN.md "Reading text tables"; what is here:
//   - structure pass: a workgroup stages one tile of DBM_TEXT_TILE_BYTES of text in LDS with 16-byte loads (lane i loads bytes 16 i ..
//     16 i + 15 of a 4 KiB slice: consecutive lanes, consecutive addresses) and leaves a newline bit per byte beside it; thread t owns the 64
//     bytes 64 t .. 64 t + 63 of the tile and every line that STARTS there.  Per tile: lines started, and how many of them are not
//     blank.  One workgroup scans the tiles' sums (the three-kernel scan of data_prims.h -- workgroup sums, one workgroup over the
//     sums, rescan -- with 64-bit counters: a file above 4 GiB can hold more than 2^32 lines);
//   - parse pass: the same staging; the rescan gives every line its index among the non-blank lines, the first skip + 1 of them are
//     left alone, line skip + 1 + k is candidate row k.  Its thread walks it out of LDS (out of global memory past the tile's end: a line
//     belongs to the tile it starts in, however long it is), converts the used fields and writes them to row k of a scratch table,
//     with a flag byte (kept / needs the host) and its byte offset;
//   - compaction: the same three-kernel scan over the flag bytes; kept candidates are copied to their final rows in file order, the
//     candidates that need the host are listed as (byte offset, final row).  No atomic append: the same bytes from call to call.
//   - the first error is the smallest byte offset of an offending line (one integer atomicMin per offending line).
// Numbers: up to 19 significant digits accumulate in a 64-bit integer w; w <= 2^53 and |e| <= 22 give double(w) * 10^e or
// double(w) / 10^-e, ONE IEEE operation on two exactly representable operands, hence correctly rounded.  Everything else that matches
// the grammar is left to the host (flag bit 1), never guessed.  All byte offsets are 64-bit.
#include "model.h"
#include "data_layouts.h"

// one rounding per operation: no fused multiply-add may appear in the conversion
#pragma clang fp contract(off)

// (in TextPair's own namespace, where the scan templates look for them)
__device__ inline TextPair operator+(TextPair x, TextPair y) { return {x.a + y.a, x.b + y.b}; }
__device__ inline TextPair operator-(TextPair x, TextPair y) { return {x.a - y.a, x.b - y.b}; }

namespace {

typedef unsigned long long u64;
constexpr int TXT_THREADS = DBM_TEXT_THREADS;
constexpr int TXT_TILE = DBM_TEXT_TILE_BYTES;
constexpr int TXT_OWN = TXT_TILE / TXT_THREADS;    // bytes of the tile whose line starts a thread owns
constexpr int TXT_SLOTS = TXT_TILE / 16;           // 16-byte loads per tile
constexpr int TXT_SCAN_ITEMS = 8;                  // consecutive candidates per lane of the compaction's scan kernels
constexpr int TXT_SCAN_TILE = TXT_THREADS * TXT_SCAN_ITEMS;
static_assert(TXT_OWN == 64, "a thread's line starts are one 64-bit mask");
static_assert(TXT_SLOTS % TXT_THREADS == 0, "every thread issues the same number of 16-byte loads");

__device__ const double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

typedef TextPair Pair64;

// one workgroup: part[t] <- exclusive scan over t; out[0], out[1] = the sums
__global__ __launch_bounds__(TXT_THREADS) void text_scan_sums_kernel(Pair64* part, long n, u64* out) {
  const Pair64 sum = scan_parts<TXT_THREADS>(part, n);
  if (threadIdx.x == 0) {
    out[0] = sum.a;
    out[1] = sum.b;
  }
}

// ---- a tile of text in LDS ----
struct TileLds {
  alignas(16) unsigned char bytes[16 + TXT_TILE];   // [15] = the byte before the tile ('\n' in front of the file), [16 ..] the tile
  unsigned short nl[TXT_SLOTS];                     // bit b of nl[s]: byte 16 s + b of the tile is '\n'
};

__device__ inline unsigned newline_bits(unsigned w) {   // bit k: byte k of w is '\n'
  unsigned m = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) m |= (((w >> (8 * k)) & 255u) == 10u ? 1u : 0u) << k;
  return m;
}

// the tile at `base` into LDS: bytes past the end of the text are zero (and never looked at: every walk stops at a.len)
__device__ void stage_tile(const TextLaunch& a, u64 base, TileLds& L) {
#pragma unroll
  for (int k = 0; k < TXT_SLOTS / TXT_THREADS; ++k) {
    const int slot = k * TXT_THREADS + (int)threadIdx.x;
    const u64 at = base + 16ull * (u64)slot;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (at + 16ull <= a.len) {
      v = *(const uint4*)(a.text + at);
    } else if (at < a.len) {
      unsigned w[4] = {0u, 0u, 0u, 0u};
      const int have = (int)(a.len - at);
      for (int j = 0; j < have; ++j) w[j >> 2] |= (unsigned)a.text[at + j] << (8 * (j & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(L.bytes + 16 + 16 * slot) = v;
    L.nl[slot] = (unsigned short)(newline_bits(v.x) | newline_bits(v.y) << 4 | newline_bits(v.z) << 8 | newline_bits(v.w) << 12);
  }
  if (threadIdx.x == 0) L.bytes[15] = base == 0ull ? (unsigned char)10 : a.text[base - 1ull];
  __syncthreads();
}

// byte p of the text, p at or behind the tile's first byte: out of LDS inside the tile, out of global memory past its end
__device__ inline unsigned char text_at(const TextLaunch& a, const TileLds& L, u64 base, u64 p) {
  const u64 d = p - base;
  return d < (u64)TXT_TILE ? L.bytes[16 + d] : a.text[p];
}

// bit i: a line starts at byte 64 t + i of the tile (the byte before it is '\n', or it is byte 0 of the file) and lies inside the text
__device__ inline u64 owned_starts(const TextLaunch& a, const TileLds& L, u64 base) {
  const int t = (int)threadIdx.x;
  const u64 first = base + (u64)(TXT_OWN * t);
  if (first >= a.len) return 0ull;
  const u64 nl = (u64)L.nl[4 * t] | (u64)L.nl[4 * t + 1] << 16 | (u64)L.nl[4 * t + 2] << 32 | (u64)L.nl[4 * t + 3] << 48;
  const u64 before = t == 0 ? (L.bytes[15] == 10 ? 1ull : 0ull) : (u64)(L.nl[4 * t - 1] >> 15);
  u64 st = (nl << 1) | before;
  const u64 rem = a.len - first;
  if (rem < 64ull) st &= (1ull << rem) - 1ull;
  return st;
}

__device__ inline bool ends_line(const TextLaunch& a, const TileLds& L, u64 base, u64 p, unsigned char c) {
  return c == 10 || (c == 13 && p + 1ull < a.len && text_at(a, L, base, p + 1ull) == 10);
}

// not blank: something other than spaces and tabs before the line's end (a tab counts when it is the separator)
__device__ bool line_has_ink(const TextLaunch& a, const TileLds& L, u64 base, u64 s) {
  for (u64 p = s; p < a.len; ++p) {
    const unsigned char c = text_at(a, L, base, p);
    if (c == ' ' || (c == '\t' && a.sep != '\t')) continue;
    return !ends_line(a, L, base, p, c);
  }
  return false;
}

// (lines, non-blank lines) that start in the calling thread's 64 bytes; *ink: bit i set for a non-blank line starting at byte i
__device__ inline Pair64 owned_lines(const TextLaunch& a, const TileLds& L, u64 base, u64 starts, u64* ink) {
  const u64 first = base + (u64)(TXT_OWN * (int)threadIdx.x);
  u64 m = 0ull;
  for (u64 rest = starts; rest; rest &= rest - 1ull) {
    const int i = __ffsll((long long)rest) - 1;
    if (line_has_ink(a, L, base, first + (u64)i)) m |= 1ull << i;
  }
  *ink = m;
  return {(u64)__popcll(starts), (u64)__popcll(m)};
}

__global__ __launch_bounds__(TXT_THREADS) void text_structure_kernel(TextLaunch a) {
  __shared__ TileLds L;
  const u64 base = (u64)blockIdx.x * (u64)TXT_TILE;
  stage_tile(a, base, L);
  u64 ink;
  Pair64 tot;
  block_exscan<TXT_THREADS>(owned_lines(a, L, base, owned_starts(a, L, base), &ink), &tot);
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = tot;
}

// ---- values ----
constexpr u64 pk(const char* s) {   // up to 8 bytes, little-endian
  u64 v = 0ull;
  for (int i = 0; i < 8 && s[i]; ++i) v |= (u64)(unsigned char)s[i] << (8 * i);
  return v;
}

// pandas' default NA strings (the empty string is handled by the caller); all are at most 8 bytes
__device__ inline bool default_na(int len, u64 lo) {
  switch (len) {
    case 2: return lo == pk("NA");
    case 3: return lo == pk("#NA") || lo == pk("N/A") || lo == pk("NaN") || lo == pk("n/a") || lo == pk("nan");
    case 4: return lo == pk("#N/A") || lo == pk("-NaN") || lo == pk("-nan") || lo == pk("<NA>") || lo == pk("NULL") || lo == pk("None") ||
                   lo == pk("null");
    case 6: return lo == pk("1.#IND");
    case 7: return lo == pk("-1.#IND") || lo == pk("1.#QNAN");
    case 8: return lo == pk("#N/A N/A") || lo == pk("-1.#QNAN");
    default: return false;
  }
}

enum { VAL_OK = 0, VAL_NAN = 1, VAL_HOST = 2, VAL_BAD = 3 };

// the field [fs, fe): trimmed of spaces and tabs, then NA strings, infinities, the number grammar
__device__ int convert_field(const TextLaunch& a, const TileLds& L, u64 base, u64 fs, u64 fe, double* value) {
  while (fs < fe) {
    const unsigned char c = text_at(a, L, base, fs);
    if (c != ' ' && c != '\t') break;
    ++fs;
  }
  while (fe > fs) {
    const unsigned char c = text_at(a, L, base, fe - 1ull);
    if (c != ' ' && c != '\t') break;
    --fe;
  }
  const u64 len = fe - fs;
  if (len == 0ull) return VAL_NAN;
  if (len <= 16ull) {
    u64 lo = 0ull, hi = 0ull;
    for (int i = 0; i < (int)len; ++i) {
      const u64 c = text_at(a, L, base, fs + (u64)i);
      if (i < 8) lo |= c << (8 * i);
      else hi |= c << (8 * (i - 8));
    }
    for (int k = 0; k < a.n_na; ++k)
      if (a.na_len[k] == (int)len && a.na_lo[k] == lo && a.na_hi[k] == hi) return VAL_NAN;
    if (hi == 0ull && default_na((int)len, lo)) return VAL_NAN;
    // [+-]?(inf|infinity), any case: bit 5 set in every byte maps letters to lower case and nothing else onto a letter
    const unsigned char c0 = (unsigned char)(lo & 255ull);
    const bool sign = c0 == '+' || c0 == '-';
    const u64 body = sign ? (lo >> 8) | (hi << 56) : lo, rest = sign ? hi >> 8 : hi;
    const int blen = (int)len - (sign ? 1 : 0);
    const u64 low = body | 0x2020202020202020ull;
    if (rest == 0ull && ((blen == 3 && low == (pk("inf") | 0x2020202020202020ull)) || (blen == 8 && low == pk("infinity")))) {
      *value = c0 == '-' ? -INFINITY : INFINITY;
      return VAL_OK;
    }
  }
  // [+-]?(digits[.digits*] | .digits)([eE][+-]?digits)?
  u64 p = fs;
  unsigned char c = text_at(a, L, base, p);
  const bool neg = c == '-';
  if (c == '+' || c == '-') ++p;
  u64 w = 0ull;
  int nd = 0, e10 = 0;
  bool many = false, any_int = false, any_frac = false;
  for (; p < fe; ++p) {
    c = text_at(a, L, base, p);
    if (c < '0' || c > '9') break;
    any_int = true;
    if (w != 0ull || c != '0') {
      if (nd < 19) { w = w * 10ull + (u64)(c - '0'); ++nd; }
      else many = true;
    }
  }
  if (p < fe && text_at(a, L, base, p) == '.') {
    for (++p; p < fe; ++p) {
      c = text_at(a, L, base, p);
      if (c < '0' || c > '9') break;
      any_frac = true;
      if (w != 0ull || c != '0') {
        if (nd < 19) { w = w * 10ull + (u64)(c - '0'); ++nd; --e10; }
        else many = true;
      } else if (e10 > -100000) {
        --e10;
      }
    }
  }
  if (!any_int && !any_frac) return VAL_BAD;
  if (p < fe) {
    c = text_at(a, L, base, p);
    if (c != 'e' && c != 'E') return VAL_BAD;
    ++p;
    bool eneg = false;
    if (p < fe) {
      c = text_at(a, L, base, p);
      eneg = c == '-';
      if (c == '+' || c == '-') ++p;
    }
    if (p >= fe) return VAL_BAD;
    int ex = 0;
    for (; p < fe; ++p) {
      c = text_at(a, L, base, p);
      if (c < '0' || c > '9') return VAL_BAD;
      if (ex < 100000) ex = ex * 10 + (int)(c - '0');
    }
    e10 += eneg ? -ex : ex;
  }
  if (many) return VAL_HOST;
  double v;
  if (w == 0ull) v = 0.0;
  else if (w <= 9007199254740992ull && e10 >= -22 && e10 <= 22) v = e10 < 0 ? (double)w / P10[-e10] : (double)w * P10[e10];
  else return VAL_HOST;
  *value = neg ? -v : v;
  return VAL_OK;
}

// the line at s is candidate row `cand`: its used fields into the scratch row, its flag byte, its offset
__device__ void parse_line(const TextLaunch& a, const TileLds& L, u64 base, u64 s, u64 cand) {
  double* row = a.rows + cand * (u64)a.nuse;
  u64 seen = 0ull;   // used fields that hold a number
  bool bad = false, host = false, done = false;
  int f = 0;
  u64 p = s;
  const bool ws = a.sep == DBM_TEXT_SEP_WHITESPACE;
  while (!done) {
    u64 fs = p, fe;
    if (ws) {
      // runs of spaces and tabs separate; leading and trailing runs are ignored
      for (; p < a.len; ++p) {
        const unsigned char c = text_at(a, L, base, p);
        if (c != ' ' && c != '\t') break;
      }
      if (p >= a.len || ends_line(a, L, base, p, text_at(a, L, base, p))) break;
      fs = p;
      for (; p < a.len; ++p) {
        const unsigned char c = text_at(a, L, base, p);
        if (c == ' ' || c == '\t' || ends_line(a, L, base, p, c)) break;
      }
      fe = p;
    } else {
      for (; p < a.len; ++p) {
        const unsigned char c = text_at(a, L, base, p);
        if (c == (unsigned char)a.sep) break;
        if (ends_line(a, L, base, p, c)) { done = true; break; }
      }
      if (p >= a.len) done = true;
      fe = p;
      ++p;   // behind the separator
    }
    if (f >= a.nfields) { bad = true; break; }   // more fields than names
    if ((a.use_mask >> f) & 1ull) {
      double v = 0.0;
      const int r = convert_field(a, L, base, fs, fe, &v);
      if (r == VAL_BAD) { bad = true; break; }
      if (r == VAL_OK) row[__popcll(a.use_mask & ((1ull << f) - 1ull))] = v;
      if (r != VAL_NAN) seen |= 1ull << f;
      host = host || r == VAL_HOST;
    }
    ++f;
  }
  const bool keep = !bad && seen == a.use_mask;
  a.flags[cand] = (unsigned char)((keep ? 1 : 0) | (keep && host ? 2 : 0));
  a.offs[cand] = s;
  if (bad) atomicMin(a.first_error, s);
}

__global__ __launch_bounds__(TXT_THREADS) void text_parse_kernel(TextLaunch a) {
  __shared__ TileLds L;
  const u64 base = (u64)blockIdx.x * (u64)TXT_TILE;
  stage_tile(a, base, L);
  const u64 starts = owned_starts(a, L, base);
  u64 ink;
  Pair64 tot;
  const Pair64 ex = block_exscan<TXT_THREADS>(owned_lines(a, L, base, starts, &ink), &tot);
  u64 rank = a.tiles[blockIdx.x].b + ex.b;   // non-blank lines in front of this thread's
  const u64 first = base + (u64)(TXT_OWN * (int)threadIdx.x);
  for (u64 rest = ink; rest; rest &= rest - 1ull) {
    const int i = __ffsll((long long)rest) - 1;
    if (rank >= a.skip1) parse_line(a, L, base, first + (u64)i, rank - a.skip1);
    ++rank;
  }
}

// ---- compaction ----
// the calling thread's TXT_SCAN_ITEMS consecutive flag bytes into k; how many are (kept, left to the host)
__device__ inline Pair64 flag_counts(const TextLaunch& a, unsigned char* k) {
  return scan_tile_items<TXT_THREADS, TXT_SCAN_ITEMS, Pair64>(a.flags, (long)a.ncand, k,
                                                             [](unsigned char f) { return Pair64{f & 1ull, (f >> 1) & 1ull}; });
}

__global__ __launch_bounds__(TXT_THREADS) void text_flag_sums_kernel(TextLaunch a) {
  unsigned char k[TXT_SCAN_ITEMS];
  Pair64 tot;
  block_exscan<TXT_THREADS>(flag_counts(a, k), &tot);
  if (threadIdx.x == 0) a.parts[blockIdx.x] = tot;
}

// kept candidates to their final rows (file order); candidates that need the host to repair[2 j] = byte offset, [2 j + 1] = final row
__global__ __launch_bounds__(TXT_THREADS) void text_compact_kernel(TextLaunch a) {
  const u64 first = (u64)scan_tile_first<TXT_THREADS, TXT_SCAN_ITEMS>();
  unsigned char k[TXT_SCAN_ITEMS];
  Pair64 tot;
  Pair64 ex = block_exscan<TXT_THREADS>(flag_counts(a, k), &tot) + a.parts[blockIdx.x];
#pragma unroll
  for (int j = 0; j < TXT_SCAN_ITEMS; ++j) {
    if (k[j] & 1) {
      const double* src = a.rows + (first + j) * (u64)a.nuse;
      double* dst = a.table + ex.a * (u64)a.nuse;
      for (int c = 0; c < a.nuse; ++c) dst[c] = src[c];
      if (k[j] & 2) {
        a.repair[2ull * ex.b] = (long long)a.offs[first + j];
        a.repair[2ull * ex.b + 1ull] = (long long)ex.a;
        ++ex.b;
      }
      ++ex.a;
    }
  }
}

// out[i, c] = in[i, a[c]], in[i, a[c]] + in[i, b[c]] or in[i, a[c]] - in[i, b[c]]
__global__ __launch_bounds__(TXT_THREADS) void text_columns_kernel(ColumnsLaunch a) {
  const u64 stride = (u64)gridDim.x * TXT_THREADS;
  for (u64 i = (u64)blockIdx.x * TXT_THREADS + threadIdx.x; i < a.n; i += stride) {
    const double* p = a.in + i * (u64)a.ncol_in;
    double* q = a.out + i * (u64)a.ncol_out;
    for (int c = 0; c < a.ncol_out; ++c) {
      const double v = p[a.a[c]];
      q[c] = a.op[c] == 1 ? v + p[a.b[c]] : a.op[c] == 2 ? v - p[a.b[c]] : v;
    }
  }
}

}  // namespace

long text_tiles(size_t nbytes) { return (long)((nbytes + TXT_TILE - 1) / TXT_TILE); }
long text_scan_tiles(size_t ncand) { return (long)((ncand + TXT_SCAN_TILE - 1) / TXT_SCAN_TILE); }

// the one layout of each workspace.  totals: 5 counters (first_error is totals[2]) in a 256-byte slot of their own
size_t text_structure_layout(TextLaunch& a, size_t nbytes, Carver c) {
  a.tiles = c.take<TextPair>((size_t)text_tiles(nbytes));
  a.totals = c.take<unsigned long long>(5);
  a.first_error = a.totals ? a.totals + 2 : nullptr;
  return c.bytes();
}
size_t text_parse_layout(TextLaunch& a, size_t ncand, int nuse, Carver c) {
  a.rows = c.take<double>(ncand * (size_t)nuse);
  a.offs = c.take<unsigned long long>(ncand);
  a.flags = c.take<unsigned char>(ncand);
  a.parts = c.take<TextPair>((size_t)text_scan_tiles(ncand));
  return c.bytes();
}

size_t text_structure_workspace(size_t nbytes) { TextLaunch a; return text_structure_layout(a, nbytes, Carver(nullptr)); }
void text_structure_carve(TextLaunch& a, void* ws) { text_structure_layout(a, a.len, Carver(ws)); }
size_t text_parse_workspace(size_t ncand, int nuse) { TextLaunch a; return text_parse_layout(a, ncand, nuse, Carver(nullptr)); }
void text_parse_carve(TextLaunch& a, void* ws) { text_parse_layout(a, a.ncand, a.nuse, Carver(ws)); }

// totals[0], [1] = lines, non-blank lines; the tiles' entries become the counts in front of each tile; totals[2] = no error yet
void launch_text_structure(const TextLaunch& a, hipStream_t s) {
  const long tiles = text_tiles(a.len);
  hipLaunchKernelGGL(text_structure_kernel, dim3((unsigned)tiles), dim3(TXT_THREADS), 0, s, a);
  hipLaunchKernelGGL(text_scan_sums_kernel, dim3(1), dim3(TXT_THREADS), 0, s, a.tiles, tiles, a.totals);
  DBM_HIP(hipMemsetAsync(a.first_error, 0xff, 8, s));
  DBM_HIP(hipGetLastError());
}

// behind launch_text_structure, with ncand = max(0, totals[1] - skip1) > 0: scratch rows, flags, offsets; totals[3], [4] = rows kept,
// rows that need the host
void launch_text_parse(const TextLaunch& a, hipStream_t s) {
  hipLaunchKernelGGL(text_parse_kernel, dim3((unsigned)text_tiles(a.len)), dim3(TXT_THREADS), 0, s, a);
  const long tiles = text_scan_tiles(a.ncand);
  hipLaunchKernelGGL(text_flag_sums_kernel, dim3((unsigned)tiles), dim3(TXT_THREADS), 0, s, a);
  hipLaunchKernelGGL(text_scan_sums_kernel, dim3(1), dim3(TXT_THREADS), 0, s, a.parts, tiles, a.totals + 3);
  DBM_HIP(hipGetLastError());
}

void launch_text_compact(const TextLaunch& a, hipStream_t s) {
  hipLaunchKernelGGL(text_compact_kernel, dim3((unsigned)text_scan_tiles(a.ncand)), dim3(TXT_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}

void launch_text_columns(const ColumnsLaunch& a, hipStream_t s) {
  if (a.n == 0) return;
  hipLaunchKernelGGL(text_columns_kernel, dim3(grid_stride_blocks((long)a.n, TXT_THREADS, 4096)), dim3(TXT_THREADS), 0, s, a);
  DBM_HIP(hipGetLastError());
}
