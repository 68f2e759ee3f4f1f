/* Writes the netCDF-4 fixtures of tests/golden/netcdf/ with libhdf5 (driven by make_netcdf_fixtures.py, which compiles this file with
 * h5cc, runs it in the output directory and turns what it prints and dumps into manifest.json and expected/NAME.VAR.npy).
 *
 * The files are marked the way the netCDF-4 library marks its own: link and attribute creation order tracked, the coordinate variables
 * made dimension scales (H5DSset_scale) and attached (H5DSattach_scale), _Netcdf4Dimid on them.  Every variable is read back with
 * H5Dread into the native form of its stored type and dumped to expected/NAME.VAR.bin: the oracle of the tests is libhdf5, not the
 * package's parser.  One JSON object per variable goes to stdout.
 *
 * All values come from a fixed linear congruential generator: the program writes the same files every time it runs. */
#include <hdf5.h>
#include <hdf5_hl.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if ((x) < 0) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint32_t lcg_state = 12345u;
static uint32_t lcg(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

static int first_variable = 1;

static hid_t create_file(const char* name, H5F_libver_t low, H5F_libver_t high, int track, hsize_t userblock) {
  hid_t fapl = H5Pcreate(H5P_FILE_ACCESS), fcpl = H5Pcreate(H5P_FILE_CREATE);
  CHECK(H5Pset_libver_bounds(fapl, low, high));
  if (track) {
    CHECK(H5Pset_link_creation_order(fcpl, H5P_CRT_ORDER_TRACKED | H5P_CRT_ORDER_INDEXED));
    CHECK(H5Pset_attr_creation_order(fcpl, H5P_CRT_ORDER_TRACKED | H5P_CRT_ORDER_INDEXED));
  }
  if (userblock) CHECK(H5Pset_userblock(fcpl, userblock));
  CHECK(H5Pset_obj_track_times(fcpl, 0));
  hid_t f = H5Fcreate(name, H5F_ACC_TRUNC, fcpl, fapl);
  CHECK(f);
  H5Pclose(fapl);
  H5Pclose(fcpl);
  return f;
}

static hid_t dataset_plist(int track) {
  hid_t p = H5Pcreate(H5P_DATASET_CREATE);
  CHECK(H5Pset_obj_track_times(p, 0));   /* as netCDF-4 does; and the files do not depend on when they were written */
  if (track) CHECK(H5Pset_attr_creation_order(p, H5P_CRT_ORDER_TRACKED | H5P_CRT_ORDER_INDEXED));
  return p;
}

static void put_attr(hid_t obj, const char* name, hid_t file_type, hid_t mem_type, hsize_t count, const void* value) {
  hid_t space = count ? H5Screate_simple(1, &count, NULL) : H5Screate(H5S_SCALAR);
  hid_t a = H5Acreate2(obj, name, file_type, space, H5P_DEFAULT, H5P_DEFAULT);
  CHECK(a);
  CHECK(H5Awrite(a, mem_type, value));
  H5Aclose(a);
  H5Sclose(space);
}

/* a float64 coordinate variable that is a dimension scale; compact: its values live in the object header */
static hid_t coordinate(hid_t f, const char* name, int n, double first, double step, int dimid, int track, int compact) {
  hsize_t dim = (hsize_t)n;
  hid_t space = H5Screate_simple(1, &dim, NULL), p = dataset_plist(track);
  if (compact) CHECK(H5Pset_layout(p, H5D_COMPACT));
  hid_t d = H5Dcreate2(f, name, H5T_IEEE_F64LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
  CHECK(d);
  double* v = (double*)malloc(sizeof(double) * n);
  for (int i = 0; i < n; ++i) v[i] = first + step * i;
  CHECK(H5Dwrite(d, H5T_NATIVE_DOUBLE, H5S_ALL, H5S_ALL, H5P_DEFAULT, v));
  free(v);
  CHECK(H5DSset_scale(d, name));
  put_attr(d, "_Netcdf4Dimid", H5T_STD_I32LE, H5T_NATIVE_INT, 0, &dimid);
  H5Pclose(p);
  H5Sclose(space);
  return d;
}

static void attach(hid_t var, hid_t y, hid_t x) {
  CHECK(H5DSattach_scale(var, y, 0));
  CHECK(H5DSattach_scale(var, x, 1));
}

/* reads `var` back through the library and dumps it; prints its manifest entry */
static void record(const char* file, const char* var, hid_t d, hid_t mem_type, size_t bytes, const char* dtype, const char* layout, const char* chunks,
                   const char* filters, const char* attrs) {
  hid_t space = H5Dget_space(d);
  hsize_t dims[4];
  int rank = H5Sget_simple_extent_dims(space, dims, NULL);
  size_t n = 1;
  for (int k = 0; k < rank; ++k) n *= dims[k];
  void* buf = malloc(n * bytes);
  CHECK(H5Dread(d, mem_type, H5S_ALL, H5S_ALL, H5P_DEFAULT, buf));
  char path[256];
  snprintf(path, sizeof path, "expected/%.*s.%s.bin", (int)(strlen(file) - 3), file, var);
  FILE* o = fopen(path, "wb");
  if (!o || fwrite(buf, bytes, n, o) != n) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
  fclose(o);
  free(buf);
  printf("%s{\"file\": \"%s\", \"variable\": \"%s\", \"shape\": [", first_variable ? "" : ",\n", file, var);
  first_variable = 0;
  for (int k = 0; k < rank; ++k) printf("%s%llu", k ? ", " : "", (unsigned long long)dims[k]);
  printf("], \"dtype\": \"%s\", \"layout\": \"%s\", \"chunks\": %s, \"filters\": %s, \"attrs\": %s}", dtype, layout, chunks, filters, attrs);
  H5Sclose(space);
}

/* HDF5's shuffle of n elements of `size` bytes */
static void shuffle(const unsigned char* src, unsigned char* dst, size_t n, size_t size) {
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < size; ++k) dst[k * n + i] = src[i * size + k];
}

/* ---- vel_chunked.nc: VX, VY float32 LE 70 x 50, chunks 32 x 16, shuffle + deflate, y descending ---- */
static void vel_chunked(void) {
  enum { H = 70, W = 50, CH = 32, CW = 16 };
  const char* file = "vel_chunked.nc";
  hid_t f = create_file(file, H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  hid_t y = coordinate(f, "y", H, 500000.0, -450.0, 0, 1, 0), x = coordinate(f, "x", W, -1000000.0, 450.0, 1, 1, 0);
  const char* names[2] = {"VX", "VY"};
  const float fills[2] = {-9999.0f, 0.0f};
  const int skip[2][2] = {{0, 2}, {-1, -1}};       /* the chunk (row, column) that is never written */
  const int direct[2][2] = {{1, 1}, {2, 0}};       /* the chunk written with H5DOwrite_chunk, deflate skipped: an inner one, one on the lower edge */
  for (int v = 0; v < 2; ++v) {
    static float data[H][W];
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        const uint32_t k = lcg();
        float val = (float)((int)(k % 200001u) - 100000) * 0.0125f;
        if (k % 17u == 0) val = fills[v];
        if (k % 19u == 1) val = v ? -0.0f : NAN;   /* VY: -0.0 equals its fill 0.0; VX: a NaN that is not its fill */
        data[r][c] = val;
      }
    hsize_t dims[2] = {H, W}, chunk[2] = {CH, CW};
    hid_t space = H5Screate_simple(2, dims, NULL), p = dataset_plist(1);
    CHECK(H5Pset_chunk(p, 2, chunk));
    CHECK(H5Pset_shuffle(p));
    CHECK(H5Pset_deflate(p, 4));
    CHECK(H5Pset_fill_value(p, H5T_NATIVE_FLOAT, &fills[v]));
    hid_t d = H5Dcreate2(f, names[v], H5T_IEEE_F32LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
    CHECK(d);
    for (int ty = 0; ty * CH < H; ++ty)
      for (int tx = 0; tx * CW < W; ++tx) {
        if (ty == skip[v][0] && tx == skip[v][1]) continue;
        if (ty == direct[v][0] && tx == direct[v][1]) {
          static float block[CH][CW];
          static unsigned char shuffled[CH * CW * 4];
          for (int r = 0; r < CH; ++r)
            for (int c = 0; c < CW; ++c)   /* beyond the dataset: values nobody may see */
              block[r][c] = (ty * CH + r < H && tx * CW + c < W) ? data[ty * CH + r][tx * CW + c] : 12345.0f;
          shuffle((const unsigned char*)block, shuffled, CH * CW, 4);
          hsize_t offset[2] = {(hsize_t)ty * CH, (hsize_t)tx * CW};
          CHECK(H5DOwrite_chunk(d, H5P_DEFAULT, 0x2u /* filter 1 of the pipeline, deflate, was not applied */, offset, sizeof shuffled, shuffled));
          continue;
        }
        hsize_t start[2] = {(hsize_t)ty * CH, (hsize_t)tx * CW};
        hsize_t count[2] = {(hsize_t)(ty * CH + CH <= H ? CH : H - ty * CH), (hsize_t)(tx * CW + CW <= W ? CW : W - tx * CW)};
        hid_t fs = H5Dget_space(d), ms = H5Screate_simple(2, dims, NULL);
        CHECK(H5Sselect_hyperslab(fs, H5S_SELECT_SET, start, NULL, count, NULL));
        CHECK(H5Sselect_hyperslab(ms, H5S_SELECT_SET, start, NULL, count, NULL));
        CHECK(H5Dwrite(d, H5T_NATIVE_FLOAT, ms, fs, H5P_DEFAULT, data));
        H5Sclose(fs);
        H5Sclose(ms);
      }
    put_attr(d, "_FillValue", H5T_IEEE_F32LE, H5T_NATIVE_FLOAT, 1, &fills[v]);
    put_attr(d, "units", H5T_C_S1, H5T_C_S1, 0, "m");   /* (a one-byte fixed-length string) */
    attach(d, y, x);
    char attrs[128];
    snprintf(attrs, sizeof attrs, "{\"_FillValue\": %.1f}", (double)fills[v]);
    record(file, names[v], d, H5T_NATIVE_FLOAT, 4, "<f4", "chunked", "[32, 16]", "[\"shuffle\", \"deflate\"]", attrs);
    H5Dclose(d);
    H5Pclose(p);
    H5Sclose(space);
  }
  record(file, "x", x, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  record(file, "y", y, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  H5Dclose(x);
  H5Dclose(y);
  H5Fclose(f);
}

/* ---- gmt_z.nc: z float32 contiguous, y ASCENDING, root node_offset = 1, NaN as _FillValue ---- */
static void gmt_z(void) {
  enum { H = 23, W = 31 };
  const char* file = "gmt_z.nc";
  hid_t f = create_file(file, H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  hid_t x = coordinate(f, "x", W, 1000.5, 2.0, 0, 1, 0), y = coordinate(f, "y", H, -3000.25, 2.0, 1, 1, 0);
  static float data[H][W];
  double range[2] = {1e30, -1e30};
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const uint32_t k = lcg();
      data[r][c] = k % 11u == 0 ? NAN : (float)(k % 90000u) * 0.05f - 2000.0f;
      if (!isnan(data[r][c])) { if (data[r][c] < range[0]) range[0] = data[r][c]; if (data[r][c] > range[1]) range[1] = data[r][c]; }
    }
  hsize_t dims[2] = {H, W};
  hid_t space = H5Screate_simple(2, dims, NULL), p = dataset_plist(1);
  const float nan = NAN;
  CHECK(H5Pset_fill_value(p, H5T_NATIVE_FLOAT, &nan));
  hid_t d = H5Dcreate2(f, "z", H5T_IEEE_F32LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
  CHECK(d);
  CHECK(H5Dwrite(d, H5T_NATIVE_FLOAT, H5S_ALL, H5S_ALL, H5P_DEFAULT, data));
  put_attr(d, "_FillValue", H5T_IEEE_F32LE, H5T_NATIVE_FLOAT, 1, &nan);
  put_attr(d, "actual_range", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, 2, range);
  attach(d, y, x);
  const int node_offset = 1;
  put_attr(f, "node_offset", H5T_STD_I32LE, H5T_NATIVE_INT, 1, &node_offset);
  put_attr(f, "Conventions", H5T_C_S1, H5T_C_S1, 0, "C");
  record(file, "z", d, H5T_NATIVE_FLOAT, 4, "<f4", "contiguous", "null", "[]", "{\"_FillValue\": NaN, \"node_offset\": 1}");
  record(file, "x", x, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  record(file, "y", y, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  H5Dclose(d); H5Dclose(x); H5Dclose(y);
  H5Pclose(p); H5Sclose(space);
  H5Fclose(f);
}

/* ---- packed_be.nc: int16 BIG-ENDIAN 20 x 19, chunks 8 x 8, deflate without shuffle, scale / offset, low bound V18 ---- */
static void packed_be(void) {
  enum { H = 20, W = 19 };
  const char* file = "packed_be.nc";
  hid_t f = create_file(file, H5F_LIBVER_V18, H5F_LIBVER_LATEST, 1, 0);
  hid_t y = coordinate(f, "y", H, 9500.0, -1000.0, 0, 1, 0), x = coordinate(f, "x", W, -9000.0, 1000.0, 1, 1, 0);
  static short data[H][W];
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const uint32_t k = lcg();
      data[r][c] = k % 13u == 0 ? (short)-32768 : (short)(int)(k % 65535u - 32767u);
    }
  hsize_t dims[2] = {H, W}, chunk[2] = {8, 8};
  hid_t space = H5Screate_simple(2, dims, NULL), p = dataset_plist(1);
  const short fill = -32768;
  const double scale = 0.1, offset = 1234.5;
  CHECK(H5Pset_chunk(p, 2, chunk));
  CHECK(H5Pset_deflate(p, 6));
  CHECK(H5Pset_fill_value(p, H5T_NATIVE_SHORT, &fill));
  hid_t d = H5Dcreate2(f, "thickness", H5T_STD_I16BE, space, H5P_DEFAULT, p, H5P_DEFAULT);
  CHECK(d);
  CHECK(H5Dwrite(d, H5T_NATIVE_SHORT, H5S_ALL, H5S_ALL, H5P_DEFAULT, data));
  put_attr(d, "_FillValue", H5T_STD_I16BE, H5T_NATIVE_SHORT, 1, &fill);
  put_attr(d, "scale_factor", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, 1, &scale);
  put_attr(d, "add_offset", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, 1, &offset);
  attach(d, y, x);
  record(file, "thickness", d, H5T_NATIVE_SHORT, 2, ">i2", "chunked", "[8, 8]", "[\"deflate\"]",
         "{\"_FillValue\": -32768, \"scale_factor\": 0.1, \"add_offset\": 1234.5}");
  record(file, "x", x, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  record(file, "y", y, H5T_NATIVE_DOUBLE, 8, "<f8", "contiguous", "null", "[]", "{}");
  H5Dclose(d); H5Dclose(x); H5Dclose(y);
  H5Pclose(p); H5Sclose(space);
  H5Fclose(f);
}

/* ---- old_style.nc: default bounds, nothing tracked (superblock 0, symbol-table root group, version-1 object headers), a 512-byte
 * user block, a uint8 and a float64 variable, coordinates in compact layout, a chunk one row high ---- */
static void old_style(void) {
  enum { H = 9, W = 13 };
  const char* file = "old_style.nc";
  hid_t f = create_file(file, H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 0, 512);
  hid_t y = coordinate(f, "y", H, 80.0, -10.0, 0, 0, 1), x = coordinate(f, "x", W, 5.0, 10.0, 1, 0, 1);
  static unsigned char mask[H][W];
  static double bed[H][W];
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const uint32_t k = lcg();
      mask[r][c] = (unsigned char)(k % 7u == 0 ? 255u : k % 5u);
      bed[r][c] = k % 9u == 0 ? -9999.0 : (double)(k % 1000003u) * 1.0000001e-3 - 400.0;
    }
  hsize_t dims[2] = {H, W};
  hid_t space = H5Screate_simple(2, dims, NULL);
  {
    hsize_t chunk[2] = {5, 7};
    hid_t p = dataset_plist(0);
    const unsigned char fill = 255;
    CHECK(H5Pset_chunk(p, 2, chunk));
    CHECK(H5Pset_deflate(p, 1));
    hid_t d = H5Dcreate2(f, "mask", H5T_STD_U8LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
    CHECK(d);
    CHECK(H5Dwrite(d, H5T_NATIVE_UCHAR, H5S_ALL, H5S_ALL, H5P_DEFAULT, mask));
    put_attr(d, "missing_value", H5T_STD_U8LE, H5T_NATIVE_UCHAR, 1, &fill);
    attach(d, y, x);
    record(file, "mask", d, H5T_NATIVE_UCHAR, 1, "|u1", "chunked", "[5, 7]", "[\"deflate\"]", "{\"missing_value\": 255}");
    H5Dclose(d); H5Pclose(p);
  }
  {
    hsize_t chunk[2] = {1, W};
    hid_t p = dataset_plist(0);
    const double fill = -9999.0, offset = 0.5;
    CHECK(H5Pset_chunk(p, 2, chunk));
    CHECK(H5Pset_shuffle(p));
    CHECK(H5Pset_deflate(p, 9));
    CHECK(H5Pset_fill_value(p, H5T_NATIVE_DOUBLE, &fill));
    hid_t d = H5Dcreate2(f, "bed", H5T_IEEE_F64LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
    CHECK(d);
    CHECK(H5Dwrite(d, H5T_NATIVE_DOUBLE, H5S_ALL, H5S_ALL, H5P_DEFAULT, bed));
    put_attr(d, "_FillValue", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, 1, &fill);
    put_attr(d, "add_offset", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, 1, &offset);
    attach(d, y, x);
    record(file, "bed", d, H5T_NATIVE_DOUBLE, 8, "<f8", "chunked", "[1, 13]", "[\"shuffle\", \"deflate\"]", "{\"_FillValue\": -9999.0, \"add_offset\": 0.5}");
    H5Dclose(d); H5Pclose(p);
  }
  record(file, "x", x, H5T_NATIVE_DOUBLE, 8, "<f8", "compact", "null", "[]", "{}");
  record(file, "y", y, H5T_NATIVE_DOUBLE, 8, "<f8", "compact", "null", "[]", "{}");
  H5Dclose(x); H5Dclose(y);
  H5Sclose(space);
  H5Fclose(f);
}

/* ---- the files that are refused ---- */
static void small_dataset(hid_t f, const char* name, hid_t type, int rank, int chunked, int fletcher, int track) {
  hsize_t dims[3] = {4, 6, 5}, chunk[3] = {2, 3, 5};
  static int zeros[4 * 6 * 5];
  hid_t space = H5Screate_simple(rank, dims, NULL), p = dataset_plist(track);
  if (chunked) CHECK(H5Pset_chunk(p, rank, chunk));
  if (fletcher) CHECK(H5Pset_fletcher32(p));
  hid_t d = H5Dcreate2(f, name, type, space, H5P_DEFAULT, p, H5P_DEFAULT);
  CHECK(d);
  CHECK(H5Dwrite(d, H5T_NATIVE_INT, H5S_ALL, H5S_ALL, H5P_DEFAULT, zeros));
  H5Dclose(d); H5Pclose(p); H5Sclose(space);
}

static void refused(void) {
  hid_t f = create_file("refused_dense_links.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  for (int k = 0; k < 9; ++k) {
    char name[8];
    snprintf(name, sizeof name, "v%d", k);
    small_dataset(f, name, H5T_IEEE_F32LE, 2, 0, 0, 1);
  }
  H5Fclose(f);
  f = create_file("refused_latest_index.nc", H5F_LIBVER_LATEST, H5F_LIBVER_LATEST, 1, 0);
  small_dataset(f, "v", H5T_IEEE_F32LE, 2, 1, 0, 1);
  H5Fclose(f);
  f = create_file("refused_fletcher32.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  small_dataset(f, "v", H5T_IEEE_F32LE, 2, 1, 1, 1);
  H5Fclose(f);
  f = create_file("refused_rank3.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  small_dataset(f, "v", H5T_IEEE_F32LE, 3, 0, 0, 1);
  H5Fclose(f);
  f = create_file("refused_uint32.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  small_dataset(f, "v", H5T_STD_U32LE, 2, 0, 0, 1);
  H5Fclose(f);
  /* nine attributes with their creation order tracked: one more than compact attribute storage holds */
  f = create_file("refused_dense_attrs.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  small_dataset(f, "v", H5T_IEEE_F32LE, 2, 0, 0, 1);
  {
    hid_t d = H5Dopen2(f, "v", H5P_DEFAULT);
    CHECK(d);
    for (int k = 0; k < 9; ++k) {
      char name[8];
      snprintf(name, sizeof name, "a%d", k);
      put_attr(d, name, H5T_STD_I32LE, H5T_NATIVE_INT, 1, &k);
    }
    H5Dclose(d);
  }
  H5Fclose(f);
  /* the data in another file (which is never written: the dataset is only created) */
  f = create_file("refused_external.nc", H5F_LIBVER_EARLIEST, H5F_LIBVER_LATEST, 1, 0);
  {
    hsize_t dims[2] = {4, 6};
    hid_t space = H5Screate_simple(2, dims, NULL), p = dataset_plist(1);
    CHECK(H5Pset_external(p, "refused_external.raw", 0, 4 * 6 * 4));
    hid_t d = H5Dcreate2(f, "v", H5T_IEEE_F32LE, space, H5P_DEFAULT, p, H5P_DEFAULT);
    CHECK(d);
    H5Dclose(d); H5Pclose(p); H5Sclose(space);
  }
  H5Fclose(f);
}

int main(void) {
  printf("[\n");
  vel_chunked();
  gmt_z();
  packed_be();
  old_style();
  refused();
  printf("\n]\n");
  return 0;
}
