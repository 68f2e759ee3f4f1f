// Stand-alone check of the data layer's workspace layouts on the CPU.  Every workspace is laid out by one function on a
// Carver (data_prims.h): on a null base it measures, on a real base it carves.  For a dozen sizes per layout (0 and 1 among them) this
// program demands that
//   - the carve on a real host buffer of exactly the measured size hands out as many bytes as the measuring pass counted (the end of the
//     last array is the end of the buffer);
//   - every array is 256-byte aligned, lies inside the buffer, and the arrays follow each other in the documented order;
//   - xxx_workspace(...) equals the measured size, and both equal the size the separate sum-of-sizes function gave before the layouts
//     were unified (the literals below: a term dropped from or added to a layout changes one of them).
// No kernel runs and no HIP call is made.  Built with AddressSanitizer and UBSan on the host side (tools/README.md):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I deepbedmap_amd/csrc -x hip tools/workspace_layout_check.cpp deepbedmap_amd/csrc/points.hip deepbedmap_amd/csrc/text.hip \
//         deepbedmap_amd/csrc/polygon.hip deepbedmap_amd/csrc/surface.hip -o workspace_layout_check
// With -DWORKSPACE_LITERALS_ONLY it needs the xxx_workspace functions alone and prints the rows of the tables (how the literals were
// made, from the sources as they were before the layouts were unified).
#include "model.h"
#ifndef WORKSPACE_LITERALS_ONLY
#include "data_layouts.h"
#endif

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct BmCase { long n, hw; size_t bytes; };
struct StructCase { size_t nbytes, bytes; };
struct ParseCase { size_t ncand; int nuse; size_t bytes; };
struct PolyCase { long n, nbins; bool staged; size_t bytes; };
struct SurfCase { long H, W; size_t bytes; };

static const BmCase BM[] = {
    {0, 1, 1280}, {1, 1, 2048}, {5, 1, 2048}, {1000, 7, 10496},
    {2047, 2048, 51456}, {2049, 2049, 52992}, {64, 4096, 51200}, {100000, 3, 802816},
    {6000000, 100000, 50782720}, {100000, 6000000, 73287936}, {12345, 524288, 6450432}, {12345, 524289, 6451200},
};
static const StructCase STRUCT[] = {
    {0, 256}, {1, 512}, {16383, 512}, {16384, 512},
    {16385, 512}, {262144, 512}, {262145, 768}, {1048576, 1280},
    {1048577, 1536}, {268435456, 262400}, {4294967296, 4194560}, {5000000000, 4883200},
};
static const ParseCase PARSE[] = {
    {0, 1, 0}, {1, 1, 1024}, {1, 3, 1024}, {7, 5, 1280},
    {255, 1, 4608}, {256, 1, 4608}, {2048, 3, 67840}, {2049, 3, 68608},
    {20000, 64, 10420480}, {524288, 3, 17305600}, {524289, 2, 13112320}, {1000000, 4, 41008128},
};
static const PolyCase POLY[] = {
    {0, 1, false, 1280}, {0, 1, true, 1280}, {1, 1, false, 1792}, {1, 2, true, 2048},
    {63, 64, false, 2048}, {64, 65, true, 4608}, {1000, 2048, false, 33536}, {1000, 2049, true, 66048},
    {1000000, 15876, false, 8191744}, {1000000, 15876, true, 40191744}, {12345, 524288, false, 6391808}, {12345, 524289, true, 6787840},
};
static const SurfCase SURF[] = {
    {0, 0, 33024}, {1, 1, 34304}, {1, 2, 34304}, {16, 64, 66816},
    {17, 65, 70144}, {100, 100, 363776}, {255, 257, 2195712}, {1000, 1000, 33033216},
    {2048, 2048, 138477824}, {513, 4097, 69394176}, {3000, 4000, 396189952}, {4097, 513, 69396736},
};

static long g_checks = 0;

static void fail(const char* what, int row, const char* why) {
  fprintf(stderr, "MISMATCH (%s, row %d): %s\n", what, row, why);
  exit(1);
}

#ifdef WORKSPACE_LITERALS_ONLY

int main() {
  for (const BmCase& c : BM) printf("BM {%ld, %ld, %zu}\n", c.n, c.hw, blockmedian_workspace(c.n, c.hw));
  for (const StructCase& c : STRUCT) printf("STRUCT {%zu, %zu}\n", c.nbytes, text_structure_workspace(c.nbytes));
  for (const ParseCase& c : PARSE) printf("PARSE {%zu, %d, %zu}\n", c.ncand, c.nuse, text_parse_workspace(c.ncand, c.nuse));
  for (const PolyCase& c : POLY) {
    PolyLaunch a;
    memset(&a, 0, sizeof(a));
    a.n = c.n;
    a.nbins = c.nbins;
    printf("POLY {%ld, %ld, %s, %zu}\n", c.n, c.nbins, c.staged ? "true" : "false", polygon_workspace(a, c.staged));
  }
  for (const SurfCase& c : SURF) printf("SURF {%ld, %ld, %zu}\n", c.H, c.W, surface_workspace(c.H, c.W));
  return 0;
}

#else

// a host buffer of exactly `bytes` bytes, 256-byte aligned as every device workspace is
struct Buffer {
  char* p;
  size_t bytes;
  explicit Buffer(size_t n) : p((char*)aligned_alloc(256, n ? n : 256)), bytes(n) {
    if (!p) { fprintf(stderr, "out of memory (%zu bytes)\n", n); exit(2); }
  }
  ~Buffer() { free(p); }
};

// the arrays in the order the layout hands them out: aligned, inside, one after the other
static void check_arrays(const char* what, int row, const Buffer& buf, const std::vector<const void*>& arrays) {
  uintptr_t prev = (uintptr_t)buf.p;
  for (const void* q : arrays) {
    const uintptr_t v = (uintptr_t)q;
    if (!q) fail(what, row, "an array was not carved");
    if (v % 256 != 0) fail(what, row, "an array is not 256-byte aligned");
    if (v < prev || v > (uintptr_t)buf.p + buf.bytes) fail(what, row, "an array lies outside the buffer or before its predecessor");
    prev = v;
    ++g_checks;
  }
}

static void check_sizes(const char* what, int row, size_t literal, size_t workspace, size_t measured, size_t carved) {
  if (measured != carved) fail(what, row, "the carve hands out another number of bytes than the measuring pass");
  if (workspace != measured) fail(what, row, "xxx_workspace is not the measured layout");
  if (measured != literal) fail(what, row, "the size differs from the one recorded before the layouts were unified");
  g_checks += 3;
}

int main() {
  int row = 0;
  for (const BmCase& c : BM) {
    BlockMedianLaunch m, a;
    const size_t measured = blockmedian_layout(m, c.n, c.hw, Carver(nullptr));
    Buffer buf(measured);
    const size_t carved = blockmedian_layout(a, c.n, c.hw, Carver(buf.p));
    check_sizes("block medians", row, c.bytes, blockmedian_workspace(c.n, c.hw), measured, carved);
    std::vector<const void*> arrays = {a.blk, a.perm, a.cnt, a.rowof, a.off, a.part, a.totals};
    for (int k = 0; k < DBM_BLOCKMEDIAN_CLASSES; ++k) arrays.push_back(a.lists[k]);
    check_arrays("block medians", row++, buf, arrays);
  }
  row = 0;
  for (const StructCase& c : STRUCT) {
    TextLaunch m, a;
    const size_t measured = text_structure_layout(m, c.nbytes, Carver(nullptr));
    Buffer buf(measured);
    const size_t carved = text_structure_layout(a, c.nbytes, Carver(buf.p));
    check_sizes("text structure", row, c.bytes, text_structure_workspace(c.nbytes), measured, carved);
    check_arrays("text structure", row, buf, {a.tiles, a.totals});
    if (a.first_error != a.totals + 2 || (char*)(a.totals + 5) > buf.p + buf.bytes) fail("text structure", row, "the counters leave the buffer");
    ++row;
  }
  row = 0;
  for (const ParseCase& c : PARSE) {
    TextLaunch m, a;
    const size_t measured = text_parse_layout(m, c.ncand, c.nuse, Carver(nullptr));
    Buffer buf(measured);
    const size_t carved = text_parse_layout(a, c.ncand, c.nuse, Carver(buf.p));
    check_sizes("text parse", row, c.bytes, text_parse_workspace(c.ncand, c.nuse), measured, carved);
    check_arrays("text parse", row++, buf, {a.rows, a.offs, a.flags, a.parts});
  }
  row = 0;
  for (const PolyCase& c : POLY) {
    PolyLaunch m, a;
    memset(&m, 0, sizeof(m));
    m.n = c.n;
    m.nbins = c.nbins;
    a = m;
    double *none = nullptr, *staged = nullptr;
    const size_t workspace = polygon_workspace(m, c.staged), measured = polygon_layout(m, c.staged, &none, Carver(nullptr));
    Buffer buf(measured);
    const size_t carved = polygon_layout(a, c.staged, &staged, Carver(buf.p));
    check_sizes("polygon", row, c.bytes, workspace, measured, carved);
    std::vector<const void*> arrays = {a.totals, a.listP, a.listB, a.cnt, a.cursor, a.off, a.part};
    if (c.staged) arrays.push_back(staged);
    else if (staged) fail("polygon", row, "a staging area nobody asked for");
    check_arrays("polygon", row++, buf, arrays);
  }
  row = 0;
  for (const SurfCase& c : SURF) {
    SurfaceArrays m, a;
    const size_t measured = surface_layout(m, c.H, c.W, Carver(nullptr));
    Buffer buf(measured);
    const size_t carved = surface_layout(a, c.H, c.W, Carver(buf.p));
    check_sizes("surface", row, c.bytes, surface_workspace(c.H, c.W), measured, carved);
    check_arrays("surface", row++, buf, {a.state, a.part, a.x, a.r, a.p, a.ap, a.mask});
  }
  printf("workspace layouts: %zu + %zu + %zu + %zu + %zu sizes, %ld checks, no mismatch\n", sizeof(BM) / sizeof(BM[0]),
         sizeof(STRUCT) / sizeof(STRUCT[0]), sizeof(PARSE) / sizeof(PARSE[0]), sizeof(POLY) / sizeof(POLY[0]), sizeof(SURF) / sizeof(SURF[0]), g_checks);
  return 0;
}

#endif
