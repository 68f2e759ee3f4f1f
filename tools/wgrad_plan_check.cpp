// Stand-alone check of the weight-gradient planner on the CPU: wgrad_layout() of deepbedmap_amd/csrc/wgrad_plan.h must
// plan what the planner planned before it was split from wgrad.hip.  No kernel runs and no HIP call is made; the operands are fake
// pointers with the alignment the real ones have.  Built with AddressSanitizer and UBSan (tools/README.md):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I deepbedmap_amd/csrc tools/wgrad_plan_check.cpp
//       -o wgrad_plan_check && ./wgrad_plan_check
//
// Descriptor sets, each for deterministic x cleared_target in {0, 1}^2:
//   - every row of WGRAD_ROWS of tests/test_gpu_conv_launches.py (operand offsets, strides and shared gradients restated below); the
//     categories and S found for them must also be the ones of that file's WGRAD_EXPECT (restated below);
//   - the trunk group of tools/wgrad_bench/trunk.cpp (N = 64) at 12 dense blocks and at 3 and 2: 42 and 28 units of the wave-DMA
//     form, either side of its <= 32-units rule;
//   - the discriminator's table of tools/wgrad_bench/discriminator.cpp at N = 64 as one batch, and with every layer twice into
//     one gradient (the fused D-step: real and fake batch).
// Compared per descriptor: category, S, groups, coutTiles, G, IB, R, nbr, BP, BPp, YS, Rin, Wst, ImgS, XS, nbands, wg_count, fast, pair_n,
// pair_direct, pair_stride, pair_next, the pair-buffer offset, and for tiny plans their owner and wg_start; per form: plans, total_wg,
// LDS bytes, fold_wgs, arena floats and both start tables; tiny_rowlen and tiny_wgs.  A mismatch prints the first differing field.
//
// HOW THE LITERALS (tools/wgrad_plan_expect.inc) WERE MADE: from the planner of the commit before the split, never from wgrad_plan.h.
// The host text of that commit's wgrad.hip (plan functions, WgradBatch::build) and its structs from dbm_internal.h were cut into a
// scratch header, with hipMalloc / hipMemset / hipMemcpy / hipFree stubbed by malloc / memset / memcpy / free (the stub records each
// allocation's size: the arena floats), and this file was compiled with -DWGRAD_PLAN_PARENT='"that header"': it then plans through
// WgradBatch::build(), reads the "uploaded" tables back and prints the include file.
#ifdef WGRAD_PLAN_PARENT
#include WGRAD_PLAN_PARENT
#else
#include "wgrad_plan.h"
#endif

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// ---- the descriptor sets ----
struct Arena {  // fake device allocations, 256-byte aligned like the real ones
  uintptr_t next = 0x10000000u;
  uintptr_t alloc(size_t floats) {
    const uintptr_t p = next;
    next += (4 * floats + 4096 + 255) & ~(uintptr_t)255;
    return p;
  }
};

static int conv_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

// One descriptor of WGRAD_ROWS: shape (N, C, H, W, O, k, stride, pad, ups); xbuf / dybuf >= 0: the operand is `xch` / `dych` channels wide and
// shared by every descriptor of the row that names the same buffer, starting at channel xc0 / dyc0; share >= 0: adds into that descriptor's gW / gb
struct Wd {
  int N, C, H, W, O, k, s, p, ups;
  float scale = 1.f;
  bool gb = true;
  int share = -1, xoff = 0;
  int xbuf = -1, xch = 0, xc0 = 0, dybuf = -1, dych = 0, dyc0 = 0;
};
static Wd wd(int N, int C, int H, int W, int O, int k, int s, int p, int ups) { Wd q{N, C, H, W, O, k, s, p, ups}; return q; }
static Wd nogb(Wd q) { q.gb = false; return q; }
static Wd xoff1(Wd q) { q.xoff = 1; return q; }
static Wd share(Wd q, int o) { q.share = o; return q; }
static Wd scaled(Wd q, float s) { q.scale = s; return q; }

static std::vector<WgradDesc> make_row(const std::vector<Wd>& row) {
  Arena A;
  std::vector<WgradDesc> out;
  uintptr_t shared_buf[4] = {0, 0, 0, 0};
  std::vector<uintptr_t> gW(row.size()), gb(row.size());
  for (size_t i = 0; i < row.size(); ++i) {
    const Wd& q = row[i];
    WgradDesc d;
    memset(&d, 0, sizeof(d));
    const int OH = conv_out(q.H << q.ups, q.k, q.s, q.p), OW = conv_out(q.W << q.ups, q.k, q.s, q.p);
    const int xch = q.xbuf >= 0 ? q.xch : q.C, dych = q.dybuf >= 0 ? q.dych : q.O;
    uintptr_t xb, yb;
    if (q.xbuf >= 0) {
      if (!shared_buf[q.xbuf]) shared_buf[q.xbuf] = A.alloc((size_t)q.N * xch * q.H * q.W);
      xb = shared_buf[q.xbuf];
    } else {
      xb = A.alloc((size_t)q.N * xch * q.H * q.W);
    }
    if (q.dybuf >= 0) {
      if (!shared_buf[q.dybuf]) shared_buf[q.dybuf] = A.alloc((size_t)q.N * dych * OH * OW);
      yb = shared_buf[q.dybuf];
    } else {
      yb = A.alloc((size_t)q.N * dych * OH * OW);
    }
    d.x = (const float*)(xb + 4 * (uintptr_t)q.xoff + 4 * (uintptr_t)q.xc0 * q.H * q.W);
    d.xsn = (long)xch * q.H * q.W; d.xsc = q.H * q.W; d.Cin = q.C; d.Hin = q.H; d.Win = q.W; d.ups = q.ups;
    d.dy = (const float*)(yb + 4 * (uintptr_t)q.dyc0 * OH * OW);
    d.dysn = (long)dych * OH * OW; d.dysc = OH * OW; d.Cout = q.O; d.OH = OH; d.OW = OW;
    d.KH = d.KW = q.k; d.stride = q.s; d.pad = q.p; d.N = q.N; d.scale = q.scale;
    if (q.share < 0) {
      gW[i] = A.alloc((size_t)q.O * q.C * q.k * q.k);
      gb[i] = q.gb ? A.alloc(q.O) : 0;
    } else {
      gW[i] = gW[q.share]; gb[i] = gb[q.share];
    }
    d.gW = (float*)gW[i]; d.gb = (float*)gb[i];
    out.push_back(d);
  }
  return out;
}

// the dense block's pattern: Cin in {64 .. 192} as prefixes of ONE 192-channel buffer, dy = 32-channel slices of another
static std::vector<Wd> trunk_row(int N, int scale_at) {
  std::vector<Wd> out;
  for (int i = 0; i < 5; ++i) {
    Wd q = wd(N, 64 + 32 * i, 9, 9, 32, 3, 1, 1, 0);
    if (i == scale_at) q.scale = 0.2f;
    q.xbuf = 0; q.xch = 192; q.xc0 = 0; q.dybuf = 1; q.dych = 192; q.dyc0 = 32 * i;
    out.push_back(q);
  }
  return out;
}

struct Triple { int cat, S_det, S_nondet; };
struct Row { const char* id; std::vector<Wd> descs; std::vector<Triple> expect; };  // expect: WGRAD_EXPECT (empty: the row has none)

static std::vector<Row> wgrad_rows() {
  std::vector<Row> R;
  R.push_back({"cat0", {wd(2, 576, 6, 6, 64, 1, 1, 0, 0), nogb(wd(3, 96, 2, 1, 32, 1, 1, 0, 0)), wd(1, 96, 1, 1, 32, 1, 1, 0, 0)},
               {{0, 1, 1}, {0, 1, 1}, {0, 1, 1}}});
  R.push_back({"cat1", {wd(2, 64, 3, 3, 64, 3, 1, 1, 1), nogb(wd(2, 64, 5, 1, 64, 3, 1, 1, 0)), xoff1(wd(3, 96, 4, 5, 32, 3, 1, 1, 0))},
               {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}}});
  R.push_back({"cat2", {nogb(wd(5, 64, 11, 9, 32, 4, 2, 1, 0)), wd(17, 96, 4, 4, 64, 4, 2, 1, 0), wd(3, 32, 7, 5, 96, 4, 2, 1, 0)},
               {{2, 2, 2}, {2, 1, 1}, {2, 1, 1}}});
  R.push_back({"cat3-n5", trunk_row(5, 4), {{3, 5, 5}, {3, 5, 5}, {3, 5, 5}, {3, 5, 5}, {3, 5, 5}}});
  {
    std::vector<Wd> v = trunk_row(9, 0);
    v.resize(3);
    v.push_back(wd(4, 32, 4, 4, 64, 3, 1, 1, 0));
    v.push_back(nogb(wd(2, 64, 9, 9, 64, 3, 1, 1, 0)));
    R.push_back({"cat3-n9", v, {{3, 9, 9}, {3, 9, 9}, {3, 9, 9}, {3, 1, 1}, {3, 2, 2}}});
  }
  R.push_back({"cat4", {wd(5, 64, 11, 13, 32, 3, 1, 1, 0), nogb(wd(2, 32, 5, 5, 64, 3, 1, 1, 1)), wd(1, 96, 12, 9, 96, 3, 1, 1, 0)},
               {{4, 5, 5}, {4, 2, 2}, {4, 1, 1}}});
  R.push_back({"cat5", {wd(2, 32, 21, 19, 64, 4, 2, 1, 0), nogb(wd(3, 64, 18, 18, 32, 4, 2, 1, 0)), wd(1, 96, 24, 20, 96, 4, 2, 1, 0)},
               {{5, 2, 2}, {5, 3, 3}, {5, 2, 2}}});
  R.push_back({"cat6", {wd(2, 64, 36, 36, 64, 3, 1, 1, 0), nogb(wd(3, 64, 23, 21, 32, 3, 1, 1, 0)), wd(1, 96, 18, 18, 96, 3, 1, 1, 0)},
               {{6, 6, 6}, {6, 4, 4}, {6, 1, 1}}});
  R.push_back({"cat7", {wd(2, 64, 18, 18, 64, 3, 1, 1, 1), nogb(wd(3, 32, 9, 9, 32, 3, 1, 1, 1)), wd(1, 96, 10, 12, 96, 3, 1, 1, 1)},
               {{7, 6, 6}, {7, 3, 3}, {7, 1, 1}}});
  R.push_back({"cat8", {wd(2, 96, 36, 36, 32, 4, 2, 1, 0), nogb(wd(3, 32, 32, 40, 64, 4, 2, 1, 0)), wd(1, 64, 36, 36, 96, 4, 2, 1, 0)},
               {{8, 2, 2}, {8, 3, 3}, {8, 1, 1}}});
  R.push_back({"cat9", {wd(2, 160, 20, 20, 96, 1, 1, 0, 0), nogb(wd(3, 64, 16, 16, 32, 1, 1, 0, 0)), wd(1, 576, 18, 18, 64, 1, 1, 0, 0)},
               {{9, 4, 4}, {9, 3, 3}, {9, 2, 2}}});
  R.push_back({"mixed", {wd(1, 96, 1, 1, 32, 1, 1, 0, 0), wd(2, 64, 18, 18, 64, 1, 1, 0, 0), wd(5, 96, 9, 9, 32, 3, 1, 1, 0),
                         nogb(wd(1, 64, 36, 36, 32, 3, 1, 1, 0)), wd(2, 64, 11, 13, 32, 3, 1, 1, 0), wd(5, 64, 9, 9, 32, 4, 2, 1, 0),
                         nogb(wd(16, 64, 4, 4, 32, 4, 2, 1, 0))},
               {{0, 1, 1}, {9, 3, 3}, {3, 5, 5}, {6, 3, 3}, {4, 2, 2}, {2, 1, 1}, {-1, 1, 1}}});
  R.push_back({"tiny-shared", {nogb(wd(16, 64, 4, 4, 32, 4, 2, 1, 0)), share(nogb(wd(16, 64, 4, 4, 32, 4, 2, 1, 0)), 0),
                               scaled(nogb(wd(37, 32, 2, 2, 64, 3, 1, 1, 0)), 0.5f), share(scaled(nogb(wd(37, 32, 2, 2, 64, 3, 1, 1, 0)), 0.5f), 2),
                               nogb(wd(21, 32, 4, 4, 32, 3, 1, 1, 0))},
               {{-1, 1, 1}, {-1, 1, 1}, {-1, 1, 1}, {-1, 1, 1}, {-1, 1, 1}}});
  R.push_back({"shared-cat3", {wd(5, 64, 9, 9, 32, 3, 1, 1, 0), share(wd(5, 64, 9, 9, 32, 3, 1, 1, 0), 0), nogb(wd(3, 96, 9, 9, 64, 3, 1, 1, 0))},
               {{3, 5, 5}, {3, 5, 5}, {3, 3, 3}}});
  {
    Wd d33 = wd(3, 64, 5, 5, 32, 3, 1, 1, 0);
    d33.dybuf = 2; d33.dych = 33; d33.dyc0 = 0;
    R.push_back({"fallback", {xoff1(wd(5, 64, 9, 9, 32, 3, 1, 1, 0)), d33, xoff1(wd(2, 64, 16, 16, 32, 1, 1, 0, 0))}, {}});
  }
  return R;
}

// tools/wgrad_bench/trunk.cpp's group: five layers per dense block on one 192-channel buffer pair, one gb per block
static std::vector<WgradDesc> trunk_bench(int nrdb) {
  const int N = 64, h = 9, w = 9, hw = 81;
  Arena A;
  const size_t bufsz = (size_t)N * 192 * hw;
  const uintptr_t x = A.alloc(bufsz * nrdb), dy = A.alloc(bufsz * nrdb), gw = A.alloc((size_t)400000 * nrdb);
  std::vector<WgradDesc> out;
  for (int j = 0; j < nrdb; ++j) {
    uintptr_t g = gw + 4 * (uintptr_t)400000 * j;
    for (int k = 0; k < 5; ++k) {
      WgradDesc d;
      memset(&d, 0, sizeof(d));
      const int cin = 64 + 32 * k, cout = k == 4 ? 64 : 32;
      d.x = (const float*)(x + 4 * bufsz * j); d.xsn = 192 * hw; d.xsc = hw; d.Cin = cin; d.Hin = h; d.Win = w;
      d.dy = (const float*)(dy + 4 * (bufsz * j + (size_t)(k == 4 ? 0 : cin) * hw)); d.dysn = 192 * hw; d.dysc = hw; d.Cout = cout; d.OH = h; d.OW = w;
      d.KH = d.KW = 3; d.stride = 1; d.pad = 1; d.N = N; d.scale = 1.f;
      d.gW = (float*)g; d.gb = (float*)(gw + 4 * ((uintptr_t)400000 * j + 399000));
      g += 4 * (uintptr_t)cout * cin * 9;
      out.push_back(d);
    }
  }
  return out;
}

// tools/wgrad_bench/discriminator.cpp's table (conv1 .. conv9, N = 64, 36 x 36 input) as one batch; twice: every layer a second
// time on other operands into the same gradient
static std::vector<WgradDesc> disc_bench(bool twice) {
  const int N = 64;
  static const int O[10] = {64, 64, 128, 128, 128, 256, 256, 512, 512, 512};
  static const int Ci[10] = {1, 64, 64, 128, 128, 128, 256, 256, 512, 512};
  static const int K[10] = {3, 4, 3, 4, 3, 4, 3, 4, 3, 4};
  static const int S[10] = {1, 2, 1, 2, 1, 2, 1, 2, 1, 2};
  int hs[11];
  hs[0] = 36; hs[1] = 36;
  for (int i = 1; i < 10; ++i) hs[i + 1] = (hs[i] + 2 - K[i]) / S[i] + 1;
  Arena A;
  const size_t big = (size_t)N * 64 * 36 * 36;
  uintptr_t x[2], dy[2];
  for (int g = 0; g < 2; ++g) { x[g] = A.alloc(big); dy[g] = A.alloc(big); }
  std::vector<WgradDesc> out;
  for (int i = 1; i < 10; ++i) {
    const uintptr_t gw = A.alloc((size_t)O[i] * Ci[i] * K[i] * K[i]);
    for (int g = 0; g < (twice ? 2 : 1); ++g) {
      WgradDesc d;
      memset(&d, 0, sizeof(d));
      const int hin = hs[i], ho = hs[i + 1];
      d.x = (const float*)x[g]; d.xsn = (long)Ci[i] * hin * hin; d.xsc = hin * hin; d.Cin = Ci[i]; d.Hin = hin; d.Win = hin;
      d.dy = (const float*)dy[g]; d.dysn = (long)O[i] * ho * ho; d.dysc = ho * ho; d.Cout = O[i]; d.OH = ho; d.OW = ho;
      d.KH = d.KW = K[i]; d.stride = S[i]; d.pad = 1; d.N = N; d.scale = 1.f; d.gW = (float*)gw; d.gb = nullptr;
      out.push_back(d);
    }
  }
  return out;
}

// ---- what a plan of a set looks like: named values in a fixed order ----
struct Record {
  std::vector<std::string> name;
  std::vector<long> value;
  void put(const std::string& n, long v) { name.push_back(n); value.push_back(v); }
};

template <class P>
static void put_plan(Record& r, const std::string& at, const P& p, long pair_off) {
  r.put(at + "groups", p.groups); r.put(at + "coutTiles", p.coutTiles); r.put(at + "G", p.G); r.put(at + "IB", p.IB); r.put(at + "R", p.R);
  r.put(at + "nbr", p.nbr); r.put(at + "BP", p.BP); r.put(at + "BPp", p.BPp); r.put(at + "YS", p.YS); r.put(at + "Rin", p.Rin);
  r.put(at + "Wst", p.Wst); r.put(at + "ImgS", p.ImgS); r.put(at + "XS", p.XS); r.put(at + "nbands", p.nbands);
  r.put(at + "wg_count", p.wg_count); r.put(at + "fast", p.fast); r.put(at + "pair_n", p.pair_n); r.put(at + "pair_direct", p.pair_direct);
  r.put(at + "pair_stride", p.pair_stride); r.put(at + "pair_next", p.pair_next); r.put(at + "pair_off", pair_off);
}

static const int NCAT = 10;

#ifdef WGRAD_PLAN_PARENT
static Record plan_set(const std::vector<WgradDesc>& ds, bool det, bool cleared) {
  g_wgrad_deterministic = det;
  WgradBatch b;
  b.cleared_target = cleared;
  for (const WgradDesc& d : ds) b.add(d);
  b.build();
  Record r;
  int seen[NCAT] = {};
  const TinyPlan* tiny = (const TinyPlan*)b.d_tiny;
  for (size_t i = 0; i < ds.size(); ++i) {
    const std::string at = "desc " + std::to_string(i) + ": ";
    const int g = b.desc_cat[i];
    r.put(at + "category", g); r.put(at + "S", b.desc_S[i]);
    r.put(at + "tiny_owner", b.tiny_owner[i]);
    if (g < 0) { r.put(at + "tiny wg_start", tiny[b.tiny_owner[i]].wg_start); continue; }
    const WgradPlan& p = b.d_plans[g][seen[g]++];
    r.put(at + "plan S", p.S);
    put_plan(r, at, p, p.pairW ? (long)(p.pairW - b.d_partial[g]) : -1L);
  }
  for (int g = 0; g < NCAT; ++g) {
    const std::string at = "form " + std::to_string(g) + ": ";
    r.put(at + "plans", b.nplans[g]); r.put(at + "total_wg", b.total_wg[g]); r.put(at + "lds", (long)b.lds[g]); r.put(at + "fold_wgs", b.fold_wgs[g]);
    r.put(at + "arena_floats", b.d_partial[g] ? (long)(stub_size(b.d_partial[g]) / sizeof(float)) : 0L);
    if (!b.nplans[g]) continue;
    const int n = b.nplans[g] + 1 + (det ? b.nplans[g] : 0);
    for (int k = 0; k < n; ++k) r.put(at + "starts[" + std::to_string(k) + "]", b.d_starts[g][k]);
  }
  r.put("tiny plans", b.n_tiny); r.put("tiny_rowlen", b.tiny_rowlen); r.put("tiny_wgs", b.tiny_wgs);
  return r;
}
#else
static Record plan_set(const std::vector<WgradDesc>& ds, bool det, bool cleared) {
  const WgradLayout L = wgrad_layout(ds, det, cleared);
  Record r;
  int seen[NCAT] = {};
  for (size_t i = 0; i < ds.size(); ++i) {
    const std::string at = "desc " + std::to_string(i) + ": ";
    const int g = L.desc_cat[i];
    r.put(at + "category", g); r.put(at + "S", L.desc_S[i]);
    r.put(at + "tiny_owner", L.tiny_owner[i]);
    if (g < 0) { r.put(at + "tiny wg_start", L.tiny[L.tiny_owner[i]].wg_start); continue; }
    const int k = seen[g]++;
    const WgradPlan& p = L.form[g].plans[k];
    r.put(at + "plan S", p.S);
    put_plan(r, at, p, L.form[g].pair_off[k]);
  }
  for (int g = 0; g < NCAT; ++g) {
    const WgradFormLayout& F = L.form[g];
    const std::string at = "form " + std::to_string(g) + ": ";
    r.put(at + "plans", (long)F.plans.size()); r.put(at + "total_wg", F.total_wg); r.put(at + "lds", (long)F.lds); r.put(at + "fold_wgs", F.fold_wgs);
    r.put(at + "arena_floats", (long)F.arena_floats);
    if (F.plans.empty()) continue;
    for (size_t k = 0; k < F.starts.size(); ++k) r.put(at + "starts[" + std::to_string(k) + "]", F.starts[k]);
  }
  r.put("tiny plans", (long)L.tiny.size()); r.put("tiny_rowlen", L.tiny_rowlen); r.put("tiny_wgs", L.tiny_wgs);
  return r;
}
#endif

struct ExpectCase { const char* id; int det, cleared; long first, count; };
#ifndef WGRAD_PLAN_PARENT
#include "wgrad_plan_expect.inc"
#endif

int main() {
  struct Set { std::string id; std::vector<WgradDesc> descs; std::vector<Triple> expect; };
  std::vector<Set> sets;
  for (const Row& row : wgrad_rows()) sets.push_back({row.id, make_row(row.descs), row.expect});
  sets.push_back({"trunk-12", trunk_bench(12), {}});
  sets.push_back({"trunk-3", trunk_bench(3), {}});
  sets.push_back({"trunk-2", trunk_bench(2), {}});
  sets.push_back({"disc", disc_bench(false), {}});
  sets.push_back({"disc-twice", disc_bench(true), {}});
  int failures = 0;
  size_t ncase = 0;
#ifdef WGRAD_PLAN_PARENT
  std::vector<long> all;
  std::string cases;
#endif
  for (const Set& s : sets)
    for (int det = 0; det < 2; ++det)
      for (int cleared = 0; cleared < 2; ++cleared, ++ncase) {
        const Record r = plan_set(s.descs, det != 0, cleared != 0);
        for (size_t i = 0; i < s.expect.size(); ++i) {  // WGRAD_EXPECT: the first two values of every descriptor's block
          long cat = 0, S = 0;
          for (size_t k = 0; k + 1 < r.name.size(); ++k)
            if (r.name[k] == "desc " + std::to_string(i) + ": category") { cat = r.value[k]; S = r.value[k + 1]; }
          const int want_S = det ? s.expect[i].S_det : s.expect[i].S_nondet;
          if (cat != s.expect[i].cat || S != want_S) {
            printf("FAIL %s det %d cleared %d desc %zu: category %ld S %ld, WGRAD_EXPECT has %d and %d\n", s.id.c_str(), det, cleared, i, cat, S,
                   s.expect[i].cat, want_S);
            ++failures;
          }
        }
#ifdef WGRAD_PLAN_PARENT
        cases += "    {\"" + s.id + "\", " + std::to_string(det) + ", " + std::to_string(cleared) + ", " + std::to_string(all.size()) + ", " +
                 std::to_string(r.value.size()) + "},\n";
        all.insert(all.end(), r.value.begin(), r.value.end());
#else
        const ExpectCase& e = EXPECT_CASES[std::min(ncase, sizeof(EXPECT_CASES) / sizeof(EXPECT_CASES[0]) - 1)];
        if (ncase >= sizeof(EXPECT_CASES) / sizeof(EXPECT_CASES[0]) || s.id != e.id || e.det != det || e.cleared != cleared) {
          printf("FAIL %s det %d cleared %d: the literal table has another case here\n", s.id.c_str(), det, cleared);
          return 1;
        }
        size_t k = 0;
        while (k < r.value.size() && k < (size_t)e.count && r.value[k] == EXPECT_VALUES[e.first + k]) ++k;
        if (k < r.value.size() || k < (size_t)e.count) {
          if (k < r.value.size() && k < (size_t)e.count)
            printf("FAIL %s det %d cleared %d: %s = %ld, before the split %ld\n", s.id.c_str(), det, cleared, r.name[k].c_str(), r.value[k],
                   EXPECT_VALUES[e.first + k]);
          else
            printf("FAIL %s det %d cleared %d: %zu values, before the split %ld\n", s.id.c_str(), det, cleared, r.value.size(), e.count);
          ++failures;
        }
#endif
      }
#ifdef WGRAD_PLAN_PARENT
  printf("// made by tools/wgrad_plan_check.cpp -DWGRAD_PLAN_PARENT from the planner before the split (see that file's header)\n");
  printf("static const long EXPECT_VALUES[] = {");
  for (size_t i = 0; i < all.size(); ++i) printf("%s%ld,", i % 32 == 0 ? "\n    " : " ", all[i]);
  printf("\n};\nstatic const ExpectCase EXPECT_CASES[] = {\n%s};\n", cases.c_str());
  if (failures) { fprintf(stderr, "the parent's planner disagrees with WGRAD_EXPECT\n"); return 1; }
  return 0;
#else
  if (ncase != sizeof(EXPECT_CASES) / sizeof(EXPECT_CASES[0])) { printf("FAIL: %zu cases planned, the literal table has others\n", ncase); ++failures; }
  printf("%s: %zu cases (descriptor sets x deterministic x cleared_target)\n", failures ? "FAILED" : "wgrad plan check ok", ncase);
  return failures ? 1 : 0;
#endif
}
