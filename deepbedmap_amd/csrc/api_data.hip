// extern "C" surface of libdbm.so (include/dbm.h), data preparation: rasters, point clouds, text tables, GeoTIFF blocks, polygons.
// Nothing here knows a model: a feature of this kind adds its entry point to this file (and to kernels.h, include/dbm.h, _lib.py).
#include "api_common.h"

extern "C" {

int dbm_grid_track(dbm_ctx* ctx, const float* grid_dev, long H, long W, const double geom[5], const double* points, size_t n,
                   int ncol, int interp, double threshold, double* z_out, double* stats, int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && geom != nullptr, "dbm_grid_track: NULL argument");
  DBM_CHECK(interp >= 0 && interp <= 2, "dbm_grid_track: interp must be 0 (nearest), 1 (bilinear) or 2 (bicubic)");
  DBM_CHECK(H >= 1 && W >= 1, "dbm_grid_track: empty grid");
  DBM_CHECK(interp == 0 || (H >= 2 && W >= 2), "dbm_grid_track: bilinear and bicubic need at least 2 x 2 nodes");
  DBM_CHECK(threshold > 0.0 && threshold <= 1.0, "dbm_grid_track: threshold must lie in (0, 1]");
  DBM_CHECK(ncol == 2 || ncol == 3, "dbm_grid_track: points have 2 (x, y) or 3 (x, y, z) columns");
  check_geometry("dbm_grid_track", geom);
  DBM_CHECK(geom[4] == 0.0 || geom[4] == 1.0, "dbm_grid_track: registration must be 0 (gridline) or 1 (pixel)");
  DBM_CHECK(n == 0 || (grid_dev != nullptr && points != nullptr), "dbm_grid_track: NULL grid or points");
  const bool reduce = ncol == 3 && stats != nullptr;
  const double half = geom[4] == 1.0 ? 0.5 : 0.0;
  TrackLaunch a;
  a.grid = grid_dev;
  a.H = H;
  a.W = W;
  a.x0 = geom[0]; a.y0 = geom[1]; a.dx = geom[2]; a.dy = geom[3];
  a.tlo = -half; a.thi = (double)(W - 1) + half;
  a.slo = -half; a.shi = (double)(H - 1) + half;
  a.n = (long)n;
  a.ncol = ncol;
  a.interp = interp;
  a.threshold = threshold;
  const bool dev = device_ptrs(flags);
  // host forms: points in stage[0], z_interpolated in stage[1]
  a.points = dev || n == 0 ? points : stage_table(ctx, 0, points, n * (size_t)ncol);
  a.z_out = nullptr;
  if (z_out && n > 0) a.z_out = dev ? z_out : stage_table(ctx, 1, nullptr, n);
  const int blocks = grid_track_blocks((long)n);
  double* dstats = ctx->track_tmp.as<double>(8 + 6 * (size_t)blocks);   // the folded statistics, then six moments per workgroup
  a.part = reduce ? dstats + 8 : nullptr;
  launch_grid_track(a, dstats, ctx->stream);
  if (!dev) {
    if (a.z_out) DBM_HIP(hipMemcpyAsync(z_out, a.z_out, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (reduce) DBM_HIP(hipMemcpyAsync(stats, dstats, 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  } else if (reduce) {
    DBM_HIP(hipMemcpyAsync(stats, dstats, 6 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  DBM_API_END
}

// ---- the distribution of the along-track errors (track_dist.hip) ----
// what the two calls share: the table checks, and the host form's points in stage[0], z_interpolated in stage[1]
static TrackErrors track_errors(dbm_ctx* ctx, const char* who, const double* points, const double* z_interpolated, size_t n, bool dev) {
  DBM_CHECK(n == 0 || (points != nullptr && z_interpolated != nullptr), std::string(who) + ": NULL points or z_interpolated");
  DBM_CHECK(n < ((size_t)1 << 40), std::string(who) + ": n must stay below 2^40 points");
  TrackErrors a;
  a.points = dev || n == 0 ? points : stage_table(ctx, 0, points, 3 * n);
  a.z_interp = dev || n == 0 ? z_interpolated : stage_table(ctx, 1, z_interpolated, n);
  a.n = (long)n;
  return a;
}

// the result of the host form leaves through stage[2]; the stream is drained for it, and before a workspace of the call's own is freed
static void track_result(dbm_ctx* ctx, void* out, const void* dresult, size_t bytes, bool dev, bool own_workspace) {
  if (!dev) DBM_HIP(hipMemcpyAsync(out, dresult, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (!dev || own_workspace) DBM_HIP(hipStreamSynchronize(ctx->stream));
}

int dbm_track_error_quantiles(dbm_ctx* ctx, const double* points, const double* z_interpolated, size_t n, const double* probabilities,
                              int count, double* quantiles_out, void* workspace_dev, int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && probabilities != nullptr && quantiles_out != nullptr, "dbm_track_error_quantiles: NULL argument");
  const bool dev = device_ptrs(flags);
  if (dev) note_device_write(ctx);
  DBM_CHECK(count >= 1 && count <= DBM_TRACK_MAX_QUANTILES, "dbm_track_error_quantiles: 1..16 probabilities per call");
  for (int k = 0; k < count; ++k)
    DBM_CHECK(probabilities[k] >= 0.0 && probabilities[k] <= 1.0, "dbm_track_error_quantiles: the probabilities must lie in [0, 1]");
  const TrackErrors a = track_errors(ctx, "dbm_track_error_quantiles", points, z_interpolated, n, dev);
  ScopedBuf own;
  void* ws = workspace_dev ? workspace_dev : own.as<char>(track_quantiles_workspace());
  double* dout = dev ? quantiles_out : stage_table(ctx, 2, nullptr, (size_t)count);
  launch_track_error_quantiles(a, probabilities, count, dout, ws, ctx->stream);
  track_result(ctx, quantiles_out, dout, sizeof(double) * (size_t)count, dev, workspace_dev == nullptr);
  DBM_API_END
}

int dbm_track_error_histogram(dbm_ctx* ctx, const double* points, const double* z_interpolated, size_t n, const double* edges, int bins,
                              int64_t* counts_out, void* workspace_dev, int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && edges != nullptr && counts_out != nullptr, "dbm_track_error_histogram: NULL argument");
  const bool dev = device_ptrs(flags);
  if (dev) note_device_write(ctx);
  DBM_CHECK(bins >= 1 && bins <= DBM_TRACK_MAX_BINS, "dbm_track_error_histogram: 1..4096 bins");
  for (int k = 0; k <= bins; ++k)
    DBM_CHECK(std::isfinite(edges[k]) && (k == 0 || edges[k] >= edges[k - 1]), "dbm_track_error_histogram: the edges must be finite and must not decrease");
  DBM_CHECK(edges[0] < edges[bins], "dbm_track_error_histogram: the range is empty (edges[0] >= edges[bins])");
  const TrackErrors a = track_errors(ctx, "dbm_track_error_histogram", points, z_interpolated, n, dev);
  ScopedBuf own;
  void* ws = workspace_dev ? workspace_dev : own.as<char>(track_histogram_workspace(bins));
  long long* dout = dev ? (long long*)counts_out : (long long*)stage_table(ctx, 2, nullptr, (size_t)bins);
  launch_track_error_histogram(a, edges, bins, dout, ws, ctx->stream);
  track_result(ctx, counts_out, dout, sizeof(int64_t) * (size_t)bins, dev, workspace_dev == nullptr);
  DBM_API_END
}

int dbm_grid_tile(dbm_ctx* ctx, const float* grid_dev, long H, long W, const double geom[4], const void* windows_host, long n, int mode,
                  double resolution, int out_h, int out_w, const double* nodata, const float* gapfiller, int fill_nan, float* out_dev,
                  size_t window_stride, int* counts_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && geom != nullptr, "dbm_grid_tile: NULL argument");
  note_device_write(ctx);
  DBM_CHECK(mode == 0 || mode == 1, "dbm_grid_tile: mode must be 0 (slicing) or 1 (bilinear)");
  DBM_CHECK(n >= 0, "dbm_grid_tile: negative number of windows");
  DBM_CHECK(out_h >= 1 && out_w >= 1, "dbm_grid_tile: empty tiles");
  DBM_CHECK((long)out_h * out_w < (1L << 31), "dbm_grid_tile: one tile must stay below 2^31 values");
  DBM_CHECK(H >= 1 && W >= 1, "dbm_grid_tile: empty raster");
  DBM_CHECK(mode == 0 || (H >= 2 && W >= 2), "dbm_grid_tile: bilinear needs at least 2 x 2 nodes");
  check_geometry("dbm_grid_tile", geom);
  DBM_CHECK(mode == 0 || (std::isfinite(resolution) && resolution > 0.0), "dbm_grid_tile: the resolution must be positive");
  DBM_CHECK(window_stride >= (size_t)out_h * (size_t)out_w, "dbm_grid_tile: the window stride is smaller than one tile");
  DBM_CHECK(n == 0 || (grid_dev != nullptr && out_dev != nullptr && windows_host != nullptr), "dbm_grid_tile: NULL raster, windows or output");
  DBM_CHECK(nodata == nullptr || std::isnan(*nodata) || std::isfinite(*nodata), "dbm_grid_tile: nodata must be finite or NaN");
  if (mode == 0) {  // a pure copy: every window must lie inside the raster
    const long* w = (const long*)windows_host;
    for (long k = 0; k < n; ++k, w += 4) {
      const long r1 = w[0] + (long)(out_h - 1) * w[2], c1 = w[1] + (long)(out_w - 1) * w[3];
      DBM_CHECK((w[2] == 1 || w[2] == -1) && (w[3] == 1 || w[3] == -1) && w[0] >= 0 && w[0] < H && r1 >= 0 && r1 < H && w[1] >= 0 &&
                    w[1] < W && c1 >= 0 && c1 < W, "dbm_grid_tile: window " + std::to_string(k) + " does not lie inside the raster");
    }
  }
  if (n > 0) {
    TileLaunch a;
    a.grid = grid_dev;
    a.H = H; a.W = W;
    a.x0 = geom[0]; a.y0 = geom[1]; a.dx = geom[2]; a.dy = geom[3];
    a.n = n;
    a.out_h = out_h; a.out_w = out_w; a.mode = mode;
    a.res = resolution;
    a.has_nodata = nodata != nullptr && !std::isnan(*nodata);   // (a NaN nodata masks nothing: data_prep.py:702)
    a.nodata = a.has_nodata ? *nodata : 0.0;
    a.nodata_band = 1e-8 + 1e-5 * std::fabs(a.nodata);
    a.has_fill = gapfiller != nullptr;
    a.fill = gapfiller ? *gapfiller : 0.0f;
    a.fill_nan = fill_nan != 0;
    a.out = out_dev;
    a.out_stride = (long)window_stride;
    a.counts = counts_dev;
    const size_t window_bytes = (size_t)n * sizeof(long[4]);   // (row0, col0, row step, col step) per window
    a.windows = ctx->stage[7].as<char>(window_bytes);
    DBM_HIP(hipMemcpyAsync(ctx->stage[7].p, windows_host, window_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (counts_dev) DBM_HIP(hipMemsetAsync(counts_dev, 0, sizeof(int) * (size_t)n, ctx->stream));
    launch_grid_tile(a, ctx->stream);
  }
  DBM_API_END
}

int dbm_grid_filled_windows(dbm_ctx* ctx, const float* grid_dev, long H, long W, int size, int step, int flip_rows, int flip_cols,
                            unsigned char* flags_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_filled_windows: NULL context");
  note_device_write(ctx);
  DBM_CHECK(size >= 2 && size % 2 == 0 && size <= FILLED_LDS_BYTES, "dbm_grid_filled_windows: the window size must be even, 2..8192");
  DBM_CHECK(step >= 1, "dbm_grid_filled_windows: the step must be positive");
  DBM_CHECK(H >= size && W >= size, "dbm_grid_filled_windows: the raster is smaller than one window");
  DBM_CHECK(grid_dev != nullptr && flags_dev != nullptr, "dbm_grid_filled_windows: NULL raster or flags");
  FilledLaunch a;
  a.grid = grid_dev;
  a.H = H; a.W = W;
  a.size = size; a.step = step;
  a.flip_rows = flip_rows != 0; a.flip_cols = flip_cols != 0;
  filled_windows_geometry(a);
  a.rowany = ctx->tile_tmp.as<unsigned char>((size_t)a.rows * (size_t)a.nx);
  a.flags = flags_dev;
  launch_filled_windows(a, ctx->stream);
  DBM_API_END
}

int dbm_grid_fill_gaps(dbm_ctx* ctx, const float* fine_dev, long H, long W, const double bounds[4], double resolution, const double* fine_nodata,
                       const float* coarse_dev, long cH, long cW, const double coarse_geom[4], float* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && bounds != nullptr && coarse_geom != nullptr, "dbm_grid_fill_gaps: NULL argument");
  note_device_write(ctx);
  DBM_CHECK(fine_dev != nullptr && coarse_dev != nullptr && out_dev != nullptr, "dbm_grid_fill_gaps: NULL raster or output");
  DBM_CHECK(H >= 1 && W >= 1 && H < (1L << 31) && W < (1L << 31), "dbm_grid_fill_gaps: H and W must lie in 1..2^31 - 1");
  DBM_CHECK(cH >= 2 && cW >= 2, "dbm_grid_fill_gaps: bilinear needs at least 2 x 2 coarse nodes");
  check_geometry("dbm_grid_fill_gaps", coarse_geom);
  DBM_CHECK(std::isfinite(bounds[0]) && std::isfinite(bounds[1]) && std::isfinite(bounds[2]) && std::isfinite(bounds[3]),
            "dbm_grid_fill_gaps: the bounds must be finite");
  DBM_CHECK(std::isfinite(resolution) && resolution > 0.0, "dbm_grid_fill_gaps: the resolution must be positive");
  DBM_CHECK(fine_nodata == nullptr || std::isnan(*fine_nodata) || std::isfinite(*fine_nodata), "dbm_grid_fill_gaps: nodata must be finite or NaN");
  DBM_CHECK((const void*)coarse_dev != (const void*)out_dev, "dbm_grid_fill_gaps: the output must not be the coarse raster");
  TileLaunch a;
  a.grid = coarse_dev;
  a.H = cH; a.W = cW;
  a.x0 = coarse_geom[0]; a.y0 = coarse_geom[1]; a.dx = coarse_geom[2]; a.dy = coarse_geom[3];
  a.n = 1;
  a.out_h = (int)H; a.out_w = (int)W; a.mode = 1;
  a.res = resolution;
  a.has_nodata = 0; a.nodata = 0.0; a.nodata_band = 0.0;   // (no gap filler: masking changes no value of dbm_grid_tile)
  a.has_fill = 0; a.fill = 0.0f; a.fill_nan = 0;
  a.out = out_dev; a.out_stride = H * W; a.counts = nullptr; a.windows = nullptr;
  const bool has = fine_nodata != nullptr && !std::isnan(*fine_nodata);
  launch_grid_fill_gaps(a, bounds, fine_dev, has ? 1 : 0, has ? (float)*fine_nodata : 0.0f, out_dev, ctx->stream);
  DBM_API_END
}

// ---- block reads: the staging dbm_tiff_decode and dbm_chunk_decode share ----
struct BlockStage {
  ScopedBuf up, table, decoded;   // this call's own, released on every path
  uint8_t* stage;                 // staged: block b at stage + b * block_stride; else its bytes at stage + offset
  const long* blocks;
  int staged;
  long block_stride;
};

// Checks the table's common columns, uploads the streams and the table and, for compression 5 (LZW) or 8 (deflate), decodes the streams
// into a staging area of their own; a block that does not decode throws status 11 before anything of the call is written.
// whole_decoded: decoded bytes must be a whole block (shuffled chunks: the byte planes are block_h * block_w apart), else the rows held
// will do.  whole_rows: StreamDecodeLaunch's.  The caller launches its row kernel on st and synchronises before st goes.
static void stage_blocks(dbm_ctx* ctx, const std::string& who, const void* streams_host, size_t streams_bytes, const int64_t* blocks_host,
                         int n_blocks, int compression, int block_w, int block_h, int bytes, bool whole_decoded, int whole_rows, BlockStage& st) {
  st.staged = compression != 1 ? 1 : 0;
  const int64_t row_bytes = (int64_t)block_w * bytes;
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t* e = blocks_host + 8 * (size_t)b;
    const std::string name = who + ": block " + std::to_string(e[5]);
    DBM_CHECK(e[0] >= 0 && e[1] >= 0 && (uint64_t)e[0] + (uint64_t)e[1] <= (uint64_t)streams_bytes, name + ": its bytes lie outside the streams");
    DBM_CHECK(e[2] >= 1 && e[2] <= block_h, name + ": its rows must lie in 1..block_h");
    DBM_CHECK(st.staged || (e[0] % 8 == 0 && e[1] >= (whole_decoded ? block_h : e[2]) * row_bytes),
              name + ": decoded bytes must be 8-byte aligned and complete");
    DBM_CHECK(e[3] > -(1L << 40) && e[3] < (1L << 40) && e[4] > -(1L << 40) && e[4] < (1L << 40), name + ": placement out of range");
  }
  st.block_stride = (block_h * row_bytes + 15) / 16 * 16;
  const size_t table_bytes = (size_t)n_blocks * sizeof(int64_t[8]);   // the block table; one status word per block lies behind it
  st.stage = st.up.as<uint8_t>(streams_bytes + 16);                   // (16 bytes of slack: the decoders load whole words)
  st.blocks = (const long*)st.table.as<uint8_t>(table_bytes + (size_t)n_blocks * sizeof(int));
  DBM_HIP(hipMemcpyAsync(st.up.p, streams_host, streams_bytes, hipMemcpyHostToDevice, ctx->stream));
  DBM_HIP(hipMemcpyAsync(st.table.p, blocks_host, table_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!st.staged) return;
  StreamDecodeLaunch d;
  d.streams = st.stage;
  d.stage = st.stage = st.decoded.as<uint8_t>((size_t)n_blocks * (size_t)st.block_stride);
  d.blocks = st.blocks;
  d.status = (int*)((uint8_t*)st.table.p + table_bytes);
  d.n_blocks = n_blocks; d.block_stride = st.block_stride; d.row_bytes = row_bytes; d.whole_rows = whole_rows;
  const std::string codec = compression == 8 ? "deflate" : "LZW";
  if (compression == 8) launch_block_inflate(d, ctx->stream);
  else launch_block_lzw(d, ctx->stream);
  std::vector<int> status((size_t)n_blocks);
  DBM_HIP(hipMemcpyAsync(status.data(), d.status, sizeof(int) * (size_t)n_blocks, hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < n_blocks; ++b)
    if (status[b] != 0)
      throw DbmError(11, who + ": block " + std::to_string(blocks_host[8 * (size_t)b + 5]) +
                             (status[b] == 1 ? ": malformed " + codec + " stream" : ": the " + codec + " stream does not decode to the block's size") +
                             "; nothing of this call was written");
}

// ---- GeoTIFF blocks -> a float32 plane (tiff_decode.hip) ----
int dbm_tiff_decode(dbm_ctx* ctx, const void* streams_host, size_t streams_bytes, const int64_t* blocks_host, int n_blocks, int compression,
                    int predictor, int sample_type, int block_w, int block_h, float* out_dev, long out_h, long out_w) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_tiff_decode: NULL context");
  note_device_write(ctx);
  DBM_CHECK(n_blocks >= 0, "dbm_tiff_decode: negative number of blocks");
  DBM_CHECK(compression == 1 || compression == 5 || compression == 8, "dbm_tiff_decode: compression must be 1 (decoded bytes), 5 (LZW) or 8 (deflate)");
  DBM_CHECK(sample_type >= 0 && sample_type <= 5, "dbm_tiff_decode: sample_type must lie in 0..5");
  const int bytes = block_sample_bytes(sample_type);
  DBM_CHECK(predictor == 1 || predictor == 2 || (predictor == 3 && sample_type >= 4), "dbm_tiff_decode: predictor must be 1, 2, or 3 with float samples");
  DBM_CHECK(block_w >= 1 && block_h >= 1 && (long)block_w * block_h * bytes < (1L << 31), "dbm_tiff_decode: a block must hold 1..2^31 - 1 bytes");
  DBM_CHECK(out_h >= 1 && out_w >= 1, "dbm_tiff_decode: empty output plane");
  DBM_CHECK(n_blocks == 0 || (streams_host != nullptr && blocks_host != nullptr && out_dev != nullptr), "dbm_tiff_decode: NULL streams, blocks or output");
  DBM_CHECK((long)n_blocks * block_h < (1L << 31), "dbm_tiff_decode: more than 2^31 block rows in one call");
  if (n_blocks == 0) return 0;
  BlockStage st;
  stage_blocks(ctx, "dbm_tiff_decode", streams_host, streams_bytes, blocks_host, n_blocks, compression, block_w, block_h, bytes, false, 0, st);
  TiffDecodeLaunch a;
  a.stage = st.stage; a.blocks = st.blocks; a.n_blocks = n_blocks; a.staged = st.staged; a.block_stride = st.block_stride;
  a.block_w = block_w; a.block_h = block_h; a.bytes = bytes; a.sample_type = sample_type; a.predictor = predictor;
  a.out = out_dev; a.out_h = out_h; a.out_w = out_w;
  launch_tiff_rows(a, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  DBM_API_END
}

// ---- netCDF chunks / row bands -> a float32 plane (nc_chunks.hip; deflate through tiff_inflate.hip) ----
int dbm_chunk_decode(dbm_ctx* ctx, const void* streams_host, size_t streams_bytes, const int64_t* blocks_host, int n_blocks, int compression,
                     int shuffle, int sample_type, int big_endian, int block_w, int block_h, int has_fill, uint64_t fill_bits, int has_scale,
                     double scale, double offset, float* out_dev, long out_h, long out_w) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_chunk_decode: NULL context");
  note_device_write(ctx);
  DBM_CHECK(n_blocks >= 0, "dbm_chunk_decode: negative number of blocks");
  DBM_CHECK(compression == 1 || compression == 8, "dbm_chunk_decode: compression must be 1 (decoded bytes) or 8 (zlib streams)");
  DBM_CHECK(shuffle == 0 || shuffle == 1, "dbm_chunk_decode: shuffle must be 0 or 1");
  DBM_CHECK(big_endian == 0 || big_endian == 1, "dbm_chunk_decode: big_endian must be 0 or 1");
  DBM_CHECK(has_fill == 0 || has_fill == 1, "dbm_chunk_decode: has_fill must be 0 or 1");
  DBM_CHECK(has_scale == 0 || has_scale == 1, "dbm_chunk_decode: has_scale must be 0 or 1");
  DBM_CHECK(sample_type >= 0 && sample_type <= 6, "dbm_chunk_decode: sample_type must lie in 0..6");
  const int bytes = block_sample_bytes(sample_type);
  DBM_CHECK(!has_fill || bytes == 8 || (fill_bits >> (8 * bytes)) == 0, "dbm_chunk_decode: fill_bits has bits beyond the sample's width");
  DBM_CHECK(block_w >= 1 && block_h >= 1 && (long)block_w * block_h * bytes < (1L << 31), "dbm_chunk_decode: a block must hold 1..2^31 - 1 bytes");
  DBM_CHECK(out_h >= 1 && out_w >= 1, "dbm_chunk_decode: empty output plane");
  DBM_CHECK(n_blocks == 0 || (streams_host != nullptr && blocks_host != nullptr && out_dev != nullptr), "dbm_chunk_decode: NULL streams, blocks or output");
  const unsigned groups = nc_chunks_groups_per_block(block_w, block_h);
  DBM_CHECK((long)n_blocks * groups < (1L << 31), "dbm_chunk_decode: more than 2^31 workgroups in one call");
  if (n_blocks == 0) return 0;
  for (int b = 0; b < n_blocks; ++b) {
    const int64_t* e = blocks_host + 8 * (size_t)b;
    DBM_CHECK(e[6] == 1 || e[6] == -1, "dbm_chunk_decode: block " + std::to_string(e[5]) + ": its row step must be +1 or -1");
  }
  BlockStage st;   // (an HDF5 chunk is always stored whole: that is the size the inflater checks)
  stage_blocks(ctx, "dbm_chunk_decode", streams_host, streams_bytes, blocks_host, n_blocks, compression, block_w, block_h, bytes, shuffle != 0,
               block_h, st);
  ChunkDecodeLaunch a;
  a.stage = st.stage; a.blocks = st.blocks; a.n_blocks = n_blocks; a.staged = st.staged; a.block_stride = st.block_stride;
  a.block_w = block_w; a.block_h = block_h; a.bytes = bytes; a.sample_type = sample_type;
  a.shuffle = shuffle; a.big_endian = big_endian;
  a.has_fill = has_fill; a.has_scale = has_scale; a.fill_bits = fill_bits; a.scale = scale; a.offset = offset;
  a.groups_per_block = groups;
  a.out = out_dev; a.out_h = out_h; a.out_w = out_w;
  launch_nc_chunks(a, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  DBM_API_END
}

// ---- what the block encoders share (dbm_tiff_encode, dbm_chunk_encode): sizes and status words down, the streams packed, one download ----
// words (ENCODE_WORDS bytes per block): the encoder's {size, status word} (8 bytes per block), then the packer's {offset, size} (16).
// encoded: the streams lie in slots of slot_cap bytes and their sizes come from the device (a status word, a size of 0 or one beyond
// the slot: status 12, `codec` names the stream); else table[2 b + 1] holds the sizes already.  The streams go to out_host one behind
// the other, each at the next even offset; the stream is drained before the call's workspace goes.
constexpr size_t ENCODE_WORDS = 24;
static void pack_streams(dbm_ctx* ctx, const std::string& who, const char* codec, long first, size_t nb, bool encoded, uint32_t* words,
                         const uint8_t* src, size_t src_stride, size_t slot_cap, std::vector<unsigned long long>& table, void* out_host,
                         size_t out_capacity, size_t* sizes_host) {
  if (encoded) {
    std::vector<uint32_t> result(2 * nb);
    DBM_HIP(hipMemcpyAsync(result.data(), words, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t b = 0; b < nb; ++b) {
      if (result[2 * b + 1] != 0 || result[2 * b] == 0 || result[2 * b] > slot_cap)
        throw DbmError(12, who + ": block " + std::to_string(first + (long)b) + ": its " + codec + " stream does not fit the slot of " +
                               std::to_string(slot_cap) + " bytes; nothing of this call was written");
      table[2 * b + 1] = result[2 * b];
    }
  }
  size_t total = 0;   // even-aligned offsets: TIFF wants its blocks on word boundaries
  for (size_t b = 0; b < nb; ++b) {
    table[2 * b] = total;
    total += (size_t)((table[2 * b + 1] + 1ull) & ~1ull);
  }
  DBM_CHECK(total <= out_capacity, who + ": the streams outgrow the output");   // (implied by the worst-case check)
  ScopedBuf packed;
  uint8_t* packed_dev = packed.as<uint8_t>(total + 16);
  unsigned long long* table_dev = (unsigned long long*)((uint8_t*)words + nb * 8);
  DBM_HIP(hipMemcpyAsync(table_dev, table.data(), nb * 16, hipMemcpyHostToDevice, ctx->stream));
  launch_tiff_pack(src, src_stride, table_dev, (int)nb, packed_dev, ctx->stream);
  DBM_HIP(hipMemcpyAsync(out_host, packed_dev, total, hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  for (size_t b = 0; b < nb; ++b) sizes_host[b] = (size_t)table[2 * b + 1];
}

// ---- a float32 plane -> GeoTIFF blocks (tiff_encode.hip) ----
int dbm_tiff_encode(dbm_ctx* ctx, const float* plane_dev, long H, long W, int sample_type, int block_h, int block_w, int tiled, int predictor,
                    int compression, long first, int n_blocks, void* out_host, size_t out_capacity, size_t* sizes_host) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_tiff_encode: NULL context");
  DBM_CHECK(plane_dev != nullptr, "dbm_tiff_encode: NULL plane");
  check_plane("dbm_tiff_encode", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  DBM_CHECK(sample_type == 1 || sample_type == 4, "dbm_tiff_encode: sample_type must be 1 (int16, by cast) or 4 (float32)");
  const int bytes = sample_type == 1 ? 2 : 4;
  DBM_CHECK(compression == 1 || compression == 5, "dbm_tiff_encode: compression must be 1 (raw bytes) or 5 (LZW)");
  DBM_CHECK(predictor == 1 || predictor == 2, "dbm_tiff_encode: predictor must be 1 or 2");
  DBM_CHECK(block_w >= 1 && block_h >= 1 && (long)block_w * block_h * bytes < (1L << 31), "dbm_tiff_encode: a block must hold 1..2^31 - 1 bytes");
  DBM_CHECK(tiled != 0 || (block_w == W && block_h <= H), "dbm_tiff_encode: strips are W wide and at most H high");
  const long blocks_x = (W + block_w - 1) / block_w, blocks_y = (H + block_h - 1) / block_h;
  DBM_CHECK(first >= 0 && n_blocks >= 0 && first + (long)n_blocks <= blocks_x * blocks_y, "dbm_tiff_encode: the block range lies outside the image's " +
                                                                                              std::to_string(blocks_x * blocks_y) + " blocks");
  DBM_CHECK((long)n_blocks * block_h < (1L << 31), "dbm_tiff_encode: more than 2^31 block rows in one call");
  DBM_CHECK(n_blocks == 0 || (out_host != nullptr && sizes_host != nullptr), "dbm_tiff_encode: NULL output or sizes");
  const bool lzw = compression == 5;
  const size_t block_bytes = (size_t)block_w * (size_t)block_h * (size_t)bytes;
  const size_t slot_cap = block_bytes * 3 / 2 + 64;   // dbm_lzw_encode_tiles' bound
  const size_t worst = lzw ? slot_cap : block_bytes;
  DBM_CHECK(out_capacity / ((worst + 1) & ~(size_t)1) >= (size_t)n_blocks, "dbm_tiff_encode: the output holds " + std::to_string(out_capacity) +
                                                                                " bytes, the worst case of " + std::to_string(n_blocks) + " blocks is " +
                                                                                std::to_string((size_t)n_blocks * ((worst + 1) & ~(size_t)1)));
  if (n_blocks == 0) return 0;
  TiffEncodeLaunch a;
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.sample_type = sample_type; a.bytes = bytes;
  a.block_h = block_h; a.block_w = block_w; a.tiled = tiled != 0;
  a.predictor = predictor;
  a.first = first; a.blocks_x = blocks_x; a.n_blocks = n_blocks;
  a.raw_stride = (long)((block_bytes + 15) / 16 * 16);
  a.slot_cap = slot_cap;
  ScopedBuf raw, slots, words;   // this call's own, released on every path
  const size_t nb = (size_t)n_blocks;
  a.raw = raw.as<uint8_t>(nb * (size_t)a.raw_stride);
  a.result = (uint32_t*)words.as<uint8_t>(nb * ENCODE_WORDS);
  launch_tiff_blocks(a, ctx->stream);
  std::vector<unsigned long long> table(2 * nb);
  if (lzw) {
    a.slots = slots.as<uint8_t>(nb * slot_cap);
    launch_tiff_lzw_encode(a, ctx->stream);
  } else {
    a.slots = nullptr;
    for (size_t b = 0; b < nb; ++b) {
      const long by = (first + (long)b) / blocks_x, left = H - by * block_h;
      const long rows = a.tiled || left > block_h ? (long)block_h : left;
      table[2 * b + 1] = (unsigned long long)rows * (unsigned long long)block_w * (unsigned long long)bytes;
    }
  }
  pack_streams(ctx, "dbm_tiff_encode", "LZW", first, nb, lzw, a.result, lzw ? a.slots : a.raw, lzw ? slot_cap : (size_t)a.raw_stride, slot_cap,
               table, out_host, out_capacity, sizes_host);
  DBM_API_END
}

// ---- a float32 plane -> netCDF-4 chunks (nc_chunks.hip; deflate through deflate_encode.hip) ----
int dbm_chunk_encode(dbm_ctx* ctx, const float* plane_dev, long H, long W, int chunk_h, int chunk_w, int row_step, int shuffle, int compression,
                     long first, int n_blocks, void* out_host, size_t out_capacity, size_t* sizes_host) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_chunk_encode: NULL context");
  DBM_CHECK(plane_dev != nullptr, "dbm_chunk_encode: NULL plane");
  check_plane("dbm_chunk_encode", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  DBM_CHECK(compression == 1 || compression == 8, "dbm_chunk_encode: compression must be 1 (the chunk's bytes) or 8 (zlib streams)");
  DBM_CHECK(shuffle == 0 || shuffle == 1, "dbm_chunk_encode: shuffle must be 0 or 1");
  DBM_CHECK(row_step == 1 || row_step == -1, "dbm_chunk_encode: the row step must be +1 or -1");
  DBM_CHECK(chunk_h >= 1 && chunk_w >= 1 && chunk_h <= H && chunk_w <= W, "dbm_chunk_encode: the chunk sides must lie in 1..H and 1..W");
  DBM_CHECK((long)chunk_h * chunk_w * 4 < (1L << 31), "dbm_chunk_encode: a chunk must hold less than 2^31 bytes");
  const long chunks_x = (W + chunk_w - 1) / chunk_w, chunks_y = (H + chunk_h - 1) / chunk_h;
  DBM_CHECK(first >= 0 && n_blocks >= 0 && first + (long)n_blocks <= chunks_x * chunks_y, "dbm_chunk_encode: the chunk range lies outside the image's " +
                                                                                               std::to_string(chunks_x * chunks_y) + " chunks");
  const unsigned groups = nc_chunks_groups_per_block(chunk_w, chunk_h);
  DBM_CHECK((long)n_blocks * groups < (1L << 31), "dbm_chunk_encode: more than 2^31 workgroups in one call");
  DBM_CHECK(n_blocks == 0 || (out_host != nullptr && sizes_host != nullptr), "dbm_chunk_encode: NULL output or sizes");
  const bool deflate = compression == 8;
  const size_t chunk_bytes = (size_t)chunk_h * (size_t)chunk_w * 4;
  const size_t slot_cap = deflate_slot(chunk_bytes);
  const size_t worst = deflate ? slot_cap : chunk_bytes;
  DBM_CHECK(out_capacity / ((worst + 1) & ~(size_t)1) >= (size_t)n_blocks, "dbm_chunk_encode: the output holds " + std::to_string(out_capacity) +
                                                                                " bytes, the worst case of " + std::to_string(n_blocks) + " chunks is " +
                                                                                std::to_string((size_t)n_blocks * ((worst + 1) & ~(size_t)1)));
  if (n_blocks == 0) return 0;
  ChunkEncodeLaunch a;
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.chunk_h = chunk_h; a.chunk_w = chunk_w;
  a.row_step = row_step; a.shuffle = shuffle;
  a.first = first; a.chunks_x = chunks_x; a.n_blocks = n_blocks;
  a.groups_per_block = groups;
  a.raw_stride = (long)((chunk_bytes + 15) / 16 * 16);
  ScopedBuf raw, slots, words;   // this call's own, released on every path
  const size_t nb = (size_t)n_blocks;
  a.raw = raw.as<uint8_t>(nb * (size_t)a.raw_stride);
  uint32_t* result = (uint32_t*)words.as<uint8_t>(nb * ENCODE_WORDS);
  launch_nc_chunk_cut(a, ctx->stream);
  std::vector<unsigned long long> table(2 * nb);
  DeflateLaunch d;
  d.raw = a.raw; d.raw_stride = (size_t)a.raw_stride; d.block_bytes = chunk_bytes; d.n_blocks = n_blocks;
  d.slots = nullptr; d.slot_cap = slot_cap; d.result = result;
  if (deflate) {
    d.slots = slots.as<uint8_t>(nb * slot_cap);
    launch_block_deflate(d, ctx->stream);
  } else {
    for (size_t b = 0; b < nb; ++b) table[2 * b + 1] = chunk_bytes;
  }
  pack_streams(ctx, "dbm_chunk_encode", "deflate", first, nb, deflate, result, deflate ? d.slots : a.raw, deflate ? slot_cap : (size_t)a.raw_stride,
               slot_cap, table, out_host, out_capacity, sizes_host);
  DBM_API_END
}

// ---- the overview pyramid of a plane (pyramid.hip) ----
int dbm_grid_overviews(dbm_ctx* ctx, const float* plane_dev, long H, long W, int sample_type, const double* nodata, int levels,
                       float* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_overviews: NULL context");
  note_device_write(ctx);
  DBM_CHECK(plane_dev != nullptr, "dbm_grid_overviews: NULL plane");
  DBM_CHECK(nodata != nullptr, "dbm_grid_overviews: NULL nodata");
  check_plane("dbm_grid_overviews", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  DBM_CHECK(sample_type == 1 || sample_type == 4, "dbm_grid_overviews: sample_type must be 1 (int16, by cast) or 4 (float32)");
  DBM_CHECK(sample_type == 4 || std::isfinite(*nodata), "dbm_grid_overviews: the nodata value of an int16 file must be finite");
  const int admits = pyramid_max_levels(H, W);
  DBM_CHECK(levels >= 0 && levels <= admits, "dbm_grid_overviews: levels must lie in 0.." + std::to_string(admits) + " for a plane of " +
                                                 std::to_string(H) + " x " + std::to_string(W));
  if (levels == 0) return 0;
  DBM_CHECK(out_dev != nullptr, "dbm_grid_overviews: NULL output");
  DBM_CHECK((const void*)plane_dev != (const void*)out_dev, "dbm_grid_overviews: the output must not be the input");
  PyramidLaunch a;
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.sample_type = sample_type;
  a.nodata = sample_type == 1 ? (float)std::trunc(*nodata) : (float)*nodata;   // int(nodata) / float32(nodata)
  a.levels = levels;
  a.out = out_dev;
  launch_grid_overviews(a, ctx->stream);
  DBM_API_END
}

// ---- colour relief and hillshade of a plane (relief.hip) ----
int dbm_grid_relief(dbm_ctx* ctx, const float* plane_dev, long H, long W, const double* edges_host, const uint8_t* colors_host, int n_slices,
                    int channels, int shade, double sin_a, double cos_a, double aspect, double mean, double sigma, double k, uint8_t* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_relief: NULL context");
  note_device_write(ctx);
  DBM_CHECK(plane_dev != nullptr && out_dev != nullptr, "dbm_grid_relief: NULL plane or output");
  DBM_CHECK(edges_host != nullptr && colors_host != nullptr, "dbm_grid_relief: NULL edges or colours");
  check_plane("dbm_grid_relief", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  DBM_CHECK(channels == 3 || channels == 4, "dbm_grid_relief: channels must be 3 (RGB) or 4 (RGBA)");
  DBM_CHECK(n_slices >= 1 && n_slices <= RELIEF_MAX_SLICES, "dbm_grid_relief: the table must hold 1..2048 slices");
  for (int i = 0; i <= n_slices; ++i)
    DBM_CHECK(std::isfinite(edges_host[i]) && (i == 0 || edges_host[i] > edges_host[i - 1]),
              "dbm_grid_relief: the edges must be finite and strictly ascending (edge " + std::to_string(i) + ")");
  if (shade) {
    DBM_CHECK(std::isfinite(mean) && std::isfinite(sigma) && std::isfinite(k), "dbm_grid_relief: mean, sigma and k must be finite");
    DBM_CHECK(sigma > 0.0, "dbm_grid_relief: sigma must be positive");
    DBM_CHECK(std::fabs(k) <= 0.63661977236758138, "dbm_grid_relief: |k| must not exceed 2 / pi (an amplitude of 1)");
    DBM_CHECK(std::isfinite(sin_a) && std::isfinite(cos_a) && std::isfinite(aspect), "dbm_grid_relief: sin_a, cos_a and aspect must be finite");
  }
  ReliefLaunch a;
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.n_slices = n_slices; a.channels = channels; a.shade = shade != 0;
  // the table travels through the context's staging buffers: edges in stage[0]; in stage[1] the 6 n bytes of slice colours
  a.edges = stage_table(ctx, 0, edges_host, (size_t)n_slices + 1);
  uint8_t* colors = ctx->stage[1].as<uint8_t>(6 * (size_t)n_slices);
  DBM_HIP(hipMemcpyAsync(colors, colors_host, 6 * (size_t)n_slices, hipMemcpyHostToDevice, ctx->stream));
  a.colors = colors;
  std::memcpy(a.bfn, colors_host + 6 * (size_t)n_slices, 9);   // B, F, N follow the slices
  a.sin_a = sin_a; a.cos_a = cos_a; a.aspect = aspect;
  a.mean = mean; a.sigma = sigma; a.k = k;
  a.out = out_dev;
  launch_grid_relief(a, ctx->stream);
  DBM_API_END
}

int dbm_grid_shade_stats(dbm_ctx* ctx, const float* plane_dev, long H, long W, double sin_a, double cos_a, double aspect, double* out_host) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_shade_stats: NULL context");
  DBM_CHECK(plane_dev != nullptr && out_host != nullptr, "dbm_grid_shade_stats: NULL plane or output");
  check_plane("dbm_grid_shade_stats", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  DBM_CHECK(std::isfinite(sin_a) && std::isfinite(cos_a) && std::isfinite(aspect), "dbm_grid_shade_stats: sin_a, cos_a and aspect must be finite");
  ReliefLaunch a{};
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.sin_a = sin_a; a.cos_a = cos_a; a.aspect = aspect;
  ScopedBuf ws;   // this call's own, released on every path
  double* stats = (double*)ws.as<char>(shade_stats_workspace(H, W));
  launch_shade_stats(a, stats, ctx->stream);
  DBM_HIP(hipMemcpyAsync(out_host, stats, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  DBM_API_END
}

// ---- an 8-bit image -> the deflated bands of a PNG (png_encode.hip; the segments through deflate_encode.hip) ----
int dbm_png_encode(dbm_ctx* ctx, const uint8_t* image_dev, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                   void* out_host, size_t out_capacity, size_t* sizes_host, uint32_t* adlers_host) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_png_encode: NULL context");
  const long bands = png_check_arguments("dbm_png_encode", image_dev, H, W, channels, filter, band_rows, first_band, n_bands, out_host,
                                         out_capacity, sizes_host, adlers_host);
  if (n_bands == 0) return 0;
  const long row_bytes = W * channels;
  const size_t band_bytes = (size_t)(band_rows < H ? band_rows : H) * (size_t)(row_bytes + 1), slot_cap = deflate_slot(band_bytes);
  const size_t nb = (size_t)n_bands;
  PngFilterLaunch a;
  a.image = image_dev;
  a.H = H; a.row_bytes = row_bytes;
  a.bpp = channels; a.filter = filter; a.band_rows = band_rows;
  a.first_band = first_band; a.n_bands = n_bands;
  a.groups_per_band = png_groups_per_band((long)band_bytes);
  a.raw_stride = (long)((band_bytes + 15) / 16 * 16);
  DBM_CHECK((long)n_bands * a.groups_per_band < (1L << 31), "dbm_png_encode: more than 2^31 workgroups in one call");
  // one workspace, carved: the filtered bands, the segments' slots, the bookkeeping words (pack_streams' 24 bytes per band, then the
  // segments' {Adler-32, length})
  ScopedBuf ws;   // this call's own, released on every path
  const size_t ws_bytes = png_workspace(nullptr, nb, (size_t)a.raw_stride, slot_cap, ENCODE_WORDS).bytes;
  const PngWorkspace carved = png_workspace(ws.as<char>(ws_bytes), nb, (size_t)a.raw_stride, slot_cap, ENCODE_WORDS);
  uint8_t *raw = carved.raw, *slots = carved.slots;
  uint32_t *words = carved.words, *segment_words = carved.segment_words;
  a.raw = raw;
  launch_png_filter(a, ctx->stream);
  DeflateLaunch d;
  d.raw = raw; d.raw_stride = (size_t)a.raw_stride; d.block_bytes = band_bytes; d.n_blocks = n_bands;
  d.slots = slots; d.slot_cap = slot_cap; d.result = words;
  d.segments = 1;
  d.segment_words = segment_words;
  if (first_band + n_bands == bands) {   // the image's last band ends the stream and may be short
    d.last_block = n_bands - 1;
    d.last_bytes = (size_t)(H - (bands - 1) * band_rows) * (size_t)(row_bytes + 1);
  }
  launch_block_deflate(d, ctx->stream);
  std::vector<unsigned long long> table(2 * nb);
  std::vector<uint32_t> seg(2 * nb);
  DBM_HIP(hipMemcpyAsync(seg.data(), segment_words, nb * 8, hipMemcpyDeviceToHost, ctx->stream));   // (drained by pack_streams)
  pack_streams(ctx, "dbm_png_encode", "deflate", first_band, nb, true, words, slots, slot_cap, slot_cap, table, out_host, out_capacity, sizes_host);
  for (size_t b = 0; b < nb; ++b) adlers_host[b] = seg[2 * b];
  DBM_API_END
}

// ---- the perspective view of a plane (perspective.hip; the host entry dbm_grid_perspective_host stands there) ----
int dbm_grid_minmax(dbm_ctx* ctx, const float* plane_dev, long H, long W, double* out_host) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_minmax: NULL context");
  DBM_CHECK(plane_dev != nullptr && out_host != nullptr, "dbm_grid_minmax: NULL plane or output");
  check_plane("dbm_grid_minmax", H, W, 1, "H W must stay below 2^31 samples", "empty plane");
  ScopedBuf ws;   // this call's own, released on every path
  double* out = (double*)ws.as<char>(grid_minmax_workspace(H, W));
  launch_grid_minmax(plane_dev, H, W, out, ctx->stream);
  DBM_HIP(hipMemcpyAsync(out_host, out, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  DBM_API_END
}

int dbm_grid_perspective(dbm_ctx* ctx, const float* plane_dev, long H, long W, const uint8_t* drape_dev, int drape_channels, const double* view_host,
                         long Wo, long Ho, const uint8_t* facade_rgba, const uint8_t* background_rgba, uint8_t* out_dev, int32_t* hits_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_perspective: NULL context");
  note_device_write(ctx);
  PerspLaunch a{};
  perspective_check_arguments("dbm_grid_perspective", plane_dev, H, W, drape_dev, drape_channels, view_host, Wo, Ho, background_rgba, out_dev, a.v);
  a.plane = plane_dev;
  a.H = H; a.W = W;
  a.drape = drape_dev;
  a.channels = drape_channels;
  a.Wo = Wo; a.Ho = Ho;
  a.facade_on = facade_rgba != nullptr;
  if (facade_rgba) std::memcpy(a.facade, facade_rgba, 4);
  std::memcpy(a.background, background_rgba, 4);
  a.out = out_dev;
  a.hits = hits_dev;
  ScopedBuf ws;   // this call's own, released on every path
  const size_t bytes = grid_perspective_workspace(a);
  launch_grid_perspective(a, bytes ? ws.as<char>(bytes) : nullptr, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  DBM_API_END
}

int dbm_grid_rescale(dbm_ctx* ctx, const float* in_dev, long H, long W, long out_h, long out_w, int order, int anti_aliasing, int clip,
                     int input_cast, float* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_rescale: NULL context");
  note_device_write(ctx);
  DBM_CHECK(order == 1 || order == 3, "dbm_grid_rescale: order must be 1 (linear) or 3 (cubic B-spline)");
  DBM_CHECK(H >= 2 && W >= 2, "dbm_grid_rescale: the input needs at least 2 x 2 nodes");
  DBM_CHECK(out_h >= 1 && out_w >= 1, "dbm_grid_rescale: empty output");
  DBM_CHECK(in_dev != nullptr && out_dev != nullptr, "dbm_grid_rescale: NULL input or output");
  DBM_CHECK((const void*)in_dev != (const void*)out_dev, "dbm_grid_rescale: the output must not be the input");
  RescaleLaunch a;
  a.in = in_dev;
  a.H = H; a.W = W; a.out_h = out_h; a.out_w = out_w;
  a.order = order;
  a.anti_aliasing = anti_aliasing != 0; a.clip = clip != 0; a.input_cast = input_cast != 0;
  a.out = out_dev;
  a.ws = ctx->resample_tmp.as<double>(grid_rescale_workspace(a));
  launch_grid_rescale(a, ctx->stream);
  DBM_API_END
}

int dbm_grid_rolling_std(dbm_ctx* ctx, const float* in_dev, long H, long W, int window, float* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr, "dbm_grid_rolling_std: NULL context");
  note_device_write(ctx);
  DBM_CHECK(window >= 1 && window <= 63 && window % 2 == 1, "dbm_grid_rolling_std: the window must be odd, 1..63");
  DBM_CHECK(H >= 1 && W >= 1, "dbm_grid_rolling_std: empty grid");
  DBM_CHECK(in_dev != nullptr && out_dev != nullptr, "dbm_grid_rolling_std: NULL input or output");
  DBM_CHECK((const void*)in_dev != (const void*)out_dev, "dbm_grid_rolling_std: the output must not be the input");
  launch_rolling_std(in_dev, H, W, window, out_dev, ctx->stream);
  DBM_API_END
}

// ---- gridding point clouds (points.hip) ----
// (table arguments without DBM_DEVICE_PTRS are staged in ctx->stage[k]: stage_table)
int dbm_points_polar_stereographic(dbm_ctx* ctx, const double* points_in, size_t n, int ncol, const double proj[6], double* points_out,
                                   int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && proj != nullptr, "dbm_points_polar_stereographic: NULL argument");
  const bool dev = device_ptrs(flags);
  if (dev) note_device_write(ctx);
  DBM_CHECK(ncol >= 2, "dbm_points_polar_stereographic: a table has at least 2 columns (longitude, latitude)");
  DBM_CHECK(n < ((size_t)1 << 31), "dbm_points_polar_stereographic: n must stay below 2^31");
  DBM_CHECK(std::isfinite(proj[0]) && proj[0] > 0.0 && std::isfinite(proj[1]) && proj[1] > 1.0,
            "dbm_points_polar_stereographic: the semi-major axis must be positive and the inverse flattening above 1");
  DBM_CHECK(proj[2] >= -90.0 && proj[2] < 0.0, "dbm_points_polar_stereographic: the latitude of true scale must lie in [-90, 0) (south-pole case)");
  DBM_CHECK(std::isfinite(proj[3]) && std::isfinite(proj[4]) && std::isfinite(proj[5]),
            "dbm_points_polar_stereographic: longitude of origin, false easting and false northing must be finite");
  DBM_CHECK(n == 0 || (points_in != nullptr && points_out != nullptr), "dbm_points_polar_stereographic: NULL table");
  if (n == 0) return 0;
  const double rad = 3.14159265358979323846 / 180.0;
  const double f = 1.0 / proj[1], e = std::sqrt(2.0 * f - f * f);
  const double cc = std::sqrt(std::pow(1.0 + e, 1.0 + e) * std::pow(1.0 - e, 1.0 - e));
  const double sf = std::sin(proj[2] * rad), esf = e * sf;
  const double tf = std::tan((45.0 + 0.5 * proj[2]) * rad) / std::pow((1.0 + esf) / (1.0 - esf), 0.5 * e);
  const double mf = std::cos(proj[2] * rad) / std::sqrt(1.0 - e * e * sf * sf);
  // phi_F = -90: m_F = t_F = 0 and the scale at the pole is taken as 1 (variant A with k0 = 1)
  const double k0 = proj[2] == -90.0 ? 1.0 : mf * cc / (2.0 * tf);
  ProjLaunch a;
  a.n = (long)n;
  a.ncol = ncol;
  a.e = e;
  a.half_e = 0.5 * e;
  a.scale = 2.0 * proj[0] * k0 / cc;
  a.lon0 = proj[3] * rad;
  a.fe = proj[4];
  a.fn = proj[5];
  a.in = points_in;
  a.out = points_out;
  if (!dev) a.in = a.out = stage_table(ctx, 0, points_in, n * (size_t)ncol);   // (projected in place)
  launch_points_project(a, ctx->stream);
  if (!dev) {
    DBM_HIP(hipMemcpyAsync(points_out, a.out, n * ncol * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  DBM_API_END
}

int dbm_points_region(dbm_ctx* ctx, const double* points, size_t n, int ncol, double increment, double* region_out, int64_t* count_out,
                      int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && region_out != nullptr && count_out != nullptr, "dbm_points_region: NULL argument");
  const bool dev = device_ptrs(flags);
  if (dev) note_device_write(ctx);
  DBM_CHECK(ncol >= 2, "dbm_points_region: a table has at least 2 columns (x, y)");
  DBM_CHECK(n < ((size_t)1 << 31), "dbm_points_region: n must stay below 2^31");
  DBM_CHECK(std::isfinite(increment) && increment > 0.0, "dbm_points_region: the increment must be positive and finite");
  DBM_CHECK(n == 0 || points != nullptr, "dbm_points_region: NULL table");
  const size_t ws = points_region_workspace((long)n);
  char* scratch = ctx->points_tmp.as<char>(ws + 64);   // (behind the workgroups' boxes: the host form's region and count)
  double* dregion = dev ? region_out : (double*)(scratch + ws);
  long long* dcount = dev ? (long long*)count_out : (long long*)(scratch + ws + 32);
  const double* dpts = dev || n == 0 ? points : stage_table(ctx, 0, points, n * (size_t)ncol);
  launch_points_region(dpts, (long)n, ncol, increment, scratch, dregion, dcount, ctx->stream);
  if (!dev) {
    DBM_HIP(hipMemcpyAsync(region_out, dregion, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipMemcpyAsync(count_out, dcount, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  DBM_API_END
}

int dbm_points_blockmedian(dbm_ctx* ctx, const double* points, size_t n, const double region[4], double spacing, double* table_out,
                           size_t table_capacity, int64_t* n_blocks_out, float* grid_dev, int* counts_dev, int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && region != nullptr && n_blocks_out != nullptr, "dbm_points_blockmedian: NULL argument");
  note_device_write(ctx);
  DBM_CHECK(n < ((size_t)1 << 31), "dbm_points_blockmedian: n must stay below 2^31");
  DBM_CHECK(std::isfinite(spacing) && spacing > 0.0, "dbm_points_blockmedian: the spacing must be positive and finite");
  DBM_CHECK(std::isfinite(region[0]) && std::isfinite(region[1]) && std::isfinite(region[2]) && std::isfinite(region[3]) &&
                region[1] >= region[0] && region[3] >= region[2], "dbm_points_blockmedian: the region must be finite with max >= min");
  const double wd = (region[1] - region[0]) / spacing, hd = (region[3] - region[2]) / spacing;
  DBM_CHECK(wd < 2147483647.0 && hd < 2147483647.0, "dbm_points_blockmedian: H W must stay below 2^31 blocks");
  const long W = (long)std::llrint(wd) + 1, H = (long)std::llrint(hd) + 1;
  check_plane("dbm_points_blockmedian", H, W, 1, "H W must stay below 2^31 blocks");
  DBM_CHECK(n == 0 || points != nullptr, "dbm_points_blockmedian: NULL table");
  DBM_CHECK(table_capacity == 0 || table_out != nullptr, "dbm_points_blockmedian: NULL table_out");
  const bool dev = device_ptrs(flags);
  BlockMedianLaunch a;
  a.n = (long)n;
  a.H = H;
  a.W = W;
  a.xmin = region[0];
  // the north edge fitted to the increment (+e): the region's own ymax when the spacing divides the region, else ymin + (H - 1) inc
  const double span = (double)(H - 1) * spacing;
  a.ymax = span == region[3] - region[2] ? region[3] : region[2] + span;
  a.inc = spacing;
  blockmedian_carve(a, ctx->points_tmp.as<char>(blockmedian_workspace(a.n, H * W)));
  a.points = dev || n == 0 ? points : stage_table(ctx, 0, points, 3 * n);   // (x, y, z)
  launch_blockmedian_count(a, ctx->stream);
  unsigned totals[1 + DBM_BLOCKMEDIAN_CLASSES];
  DBM_HIP(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  const size_t m = totals[0];
  DBM_CHECK(m <= table_capacity, "dbm_points_blockmedian: the table holds " + std::to_string(table_capacity) + " rows, " +
                                     std::to_string(m) + " blocks are not empty; nothing was written");
  a.table = dev ? table_out : stage_table(ctx, 1, nullptr, 3 * m);
  a.grid = grid_dev;
  a.counts = counts_dev;
  launch_blockmedian_select(a, totals, ctx->stream);
  *n_blocks_out = (int64_t)m;
  if (!dev) {
    if (m > 0) DBM_HIP(hipMemcpyAsync(table_out, a.table, 3 * m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  DBM_API_END
}

// ---- reading survey text tables (text.hip) ----
static void text_arguments(const char* who, dbm_ctx* ctx, const void* text, size_t nbytes, int separator, int flags) {
  const std::string w(who);
  DBM_CHECK(ctx != nullptr, w + ": NULL context");
  DBM_CHECK(separator == ',' || separator == '\t' || separator == DBM_TEXT_SEP_WHITESPACE,
            w + ": the separator must be ',', a tab or DBM_TEXT_SEP_WHITESPACE");
  DBM_CHECK(nbytes == 0 || text != nullptr, w + ": NULL text");
  DBM_CHECK(!device_ptrs(flags) || ((uintptr_t)text & 15) == 0, w + ": a device text pointer must be 16-byte aligned");
}

// the text on the device (host text: staged in `staged`, released with it) and the structure pass behind it; totals = {lines, non-blank}
static void text_structure(dbm_ctx* ctx, TextLaunch& a, const void* text, size_t nbytes, int separator, int flags, ScopedBuf& staged,
                           unsigned long long totals[2]) {
  a.len = nbytes;
  a.sep = separator;
  if (device_ptrs(flags)) {
    a.text = (const unsigned char*)text;
  } else {
    a.text = staged.as<unsigned char>(nbytes + 16);   // (16 bytes of slack: the kernels load whole 16-byte words)
    DBM_HIP(hipMemcpyAsync(staged.p, text, nbytes, hipMemcpyHostToDevice, ctx->stream));
  }
  text_structure_carve(a, ctx->points_tmp.as<char>(text_structure_workspace(nbytes)));
  launch_text_structure(a, ctx->stream);
  DBM_HIP(hipMemcpyAsync(totals, a.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));
}

int dbm_text_count_lines(dbm_ctx* ctx, const void* text, size_t nbytes, int separator, int64_t* counts_out, int flags) {
  DBM_API_BEGIN(ctx)
  text_arguments("dbm_text_count_lines", ctx, text, nbytes, separator, flags);
  DBM_CHECK(counts_out != nullptr, "dbm_text_count_lines: NULL counts_out");
  counts_out[0] = counts_out[1] = 0;
  if (nbytes == 0) return 0;
  TextLaunch a = {};
  ScopedBuf staged;
  unsigned long long totals[2];
  text_structure(ctx, a, text, nbytes, separator, flags, staged, totals);
  counts_out[0] = (int64_t)totals[0];
  counts_out[1] = (int64_t)totals[1];
  DBM_API_END
}

int dbm_text_parse(dbm_ctx* ctx, const void* text, size_t nbytes, int separator, int skip, int nfields, uint64_t use_mask,
                   const char* na_values, int n_na, double* table_out, size_t table_capacity, int64_t* repair_out, size_t repair_capacity,
                   int64_t* result_out, int flags) {
  DBM_API_BEGIN(ctx)
  text_arguments("dbm_text_parse", ctx, text, nbytes, separator, flags);
  note_device_write(ctx);
  DBM_CHECK(result_out != nullptr, "dbm_text_parse: NULL result_out");
  DBM_CHECK(skip >= 0, "dbm_text_parse: skip must not be negative");
  DBM_CHECK(nfields >= 1 && nfields <= DBM_TEXT_MAX_FIELDS, "dbm_text_parse: nfields must lie in 1..DBM_TEXT_MAX_FIELDS");
  DBM_CHECK(use_mask != 0 && (nfields == 64 || (use_mask >> nfields) == 0), "dbm_text_parse: use_mask must mark at least one of the nfields fields and no other");
  DBM_CHECK(n_na >= 0 && n_na <= DBM_TEXT_MAX_NA && (n_na == 0 || na_values != nullptr), "dbm_text_parse: n_na must lie in 0..DBM_TEXT_MAX_NA");
  DBM_CHECK(table_capacity == 0 || table_out != nullptr, "dbm_text_parse: NULL table_out");
  DBM_CHECK(repair_capacity == 0 || repair_out != nullptr, "dbm_text_parse: NULL repair_out");
  TextLaunch a = {};
  a.skip1 = (unsigned long long)skip + 1ull;
  a.nfields = nfields;
  a.use_mask = use_mask;
  a.nuse = __builtin_popcountll(use_mask);
  a.n_na = n_na;
  for (int k = 0; k < n_na; ++k) {
    const size_t len = strlen(na_values);
    DBM_CHECK(len >= 1 && len <= DBM_TEXT_MAX_NA_BYTES, "dbm_text_parse: an NA string must hold 1..DBM_TEXT_MAX_NA_BYTES bytes");
    a.na_len[k] = (int)len;
    for (size_t i = 0; i < len; ++i)
      (i < 8 ? a.na_lo[k] : a.na_hi[k]) |= (unsigned long long)(unsigned char)na_values[i] << (8 * (i & 7));
    na_values += len + 1;
  }
  result_out[0] = result_out[1] = result_out[3] = 0;
  result_out[2] = -1;
  if (nbytes == 0) return 0;
  const bool dev = device_ptrs(flags);
  ScopedBuf staged, scratch, list, table;
  unsigned long long totals[5];
  text_structure(ctx, a, text, nbytes, separator, flags, staged, totals);
  if (totals[1] < a.skip1) return 0;
  a.ncand = totals[1] - a.skip1;
  result_out[3] = (int64_t)a.ncand;
  if (a.ncand == 0) return 0;
  text_parse_carve(a, scratch.as<char>(text_parse_workspace(a.ncand, a.nuse)));
  launch_text_parse(a, ctx->stream);
  DBM_HIP(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  if (totals[2] != ~0ull) {
    result_out[2] = (int64_t)totals[2];
    return 0;
  }
  const size_t kept = totals[3], nrep = totals[4];
  DBM_CHECK(kept <= table_capacity, "dbm_text_parse: the table holds " + std::to_string(table_capacity) + " rows, " + std::to_string(kept) +
                                        " are kept; nothing was written");
  DBM_CHECK(nrep <= repair_capacity, "dbm_text_parse: the repair list holds " + std::to_string(repair_capacity) + " pairs, " +
                                         std::to_string(nrep) + " are needed; nothing was written");
  if (kept > 0) {
    const size_t cells = kept * (size_t)a.nuse, pair_bytes = sizeof(long long[2]);
    a.repair = (long long*)list.as<char>((nrep > 0 ? nrep : 1) * pair_bytes);
    a.table = dev ? table_out : table.as<double>(cells);
    launch_text_compact(a, ctx->stream);
    if (nrep > 0) DBM_HIP(hipMemcpyAsync(repair_out, a.repair, nrep * pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev) DBM_HIP(hipMemcpyAsync(table_out, a.table, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  result_out[0] = (int64_t)kept;
  result_out[1] = (int64_t)nrep;
  DBM_API_END
}

int dbm_text_columns(dbm_ctx* ctx, const double* in_dev, size_t n, int ncol_in, double* out_dev, int ncol_out, const int* a, const int* op,
                     const int* b) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && a != nullptr && op != nullptr && b != nullptr, "dbm_text_columns: NULL argument");
  note_device_write(ctx);
  DBM_CHECK(ncol_in >= 1 && ncol_out >= 1 && ncol_out <= DBM_TEXT_MAX_COLUMNS, "dbm_text_columns: ncol_in >= 1 and ncol_out in 1..DBM_TEXT_MAX_COLUMNS");
  DBM_CHECK(n == 0 || (in_dev != nullptr && out_dev != nullptr), "dbm_text_columns: NULL table");
  ColumnsLaunch c = {};
  c.in = in_dev;
  c.out = out_dev;
  c.n = n;
  c.ncol_in = ncol_in;
  c.ncol_out = ncol_out;
  for (int k = 0; k < ncol_out; ++k) {
    DBM_CHECK(op[k] >= 0 && op[k] <= 2, "dbm_text_columns: op must be 0 (copy), 1 (add) or 2 (subtract)");
    DBM_CHECK(a[k] >= 0 && a[k] < ncol_in && (op[k] == 0 || (b[k] >= 0 && b[k] < ncol_in)), "dbm_text_columns: a column index lies outside the input");
    c.a[k] = a[k];
    c.op[k] = op[k];
    c.b[k] = op[k] == 0 ? a[k] : b[k];
  }
  launch_text_columns(c, ctx->stream);
  DBM_API_END
}

// ---- from block medians to the 250 m raster (surface.hip, track.hip) ----
int dbm_grid_tension_surface(dbm_ctx* ctx, const float* data_dev, long H, long W, double tension, double tol, int max_iter, float* out_dev,
                             double info[4]) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && data_dev != nullptr && out_dev != nullptr && info != nullptr, "dbm_grid_tension_surface: NULL argument");
  note_device_write(ctx);
  check_plane("dbm_grid_tension_surface", H, W, 3, "H W must stay below 2^31 nodes", "the raster needs at least 3 x 3 nodes");
  DBM_CHECK(tension > 0.0 && tension <= 1.0, "dbm_grid_tension_surface: the tension must lie in (0, 1]");
  DBM_CHECK(tol > 0.0 && tol < 1.0, "dbm_grid_tension_surface: tol must lie in (0, 1)");
  DBM_CHECK(max_iter >= 1 && max_iter <= 1000000, "dbm_grid_tension_surface: max_iter must lie in 1..1000000");
  ScopedBuf ws;   // this call's own: x, r, p, Ap (float64 planes), the free-node mask, the partial sums; released on every path
  SurfaceLaunch a;
  a.data = data_dev;
  a.H = H; a.W = W;
  a.tension = tension; a.tol = tol;
  a.max_iter = max_iter;
  a.out = out_dev;
  const bool converged = surface_solve(a, ws.as<char>(surface_workspace(H, W)), ctx->stream, info);
  if (!converged)
    throw DbmError(10, "dbm_grid_tension_surface: not converged in " + std::to_string(max_iter) + " iterations (relative residual " +
                           std::to_string(info[1]) + ", tol " + std::to_string(tol) + "); out_dev holds the last iterate");
  DBM_API_END
}

int dbm_grid_distance_mask(dbm_ctx* ctx, const float* data_dev, float* grid_dev, long H, long W, int radius) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && data_dev != nullptr && grid_dev != nullptr, "dbm_grid_distance_mask: NULL argument");
  note_device_write(ctx);
  check_plane("dbm_grid_distance_mask", H, W, 1, "H W must lie in 1..2^31 - 1");
  DBM_CHECK(radius >= 0 && radius <= 32, "dbm_grid_distance_mask: the radius must lie in 0..32 nodes");
  DBM_CHECK((const void*)data_dev != (const void*)grid_dev, "dbm_grid_distance_mask: the grid must not be the data raster");
  launch_distance_mask(data_dev, grid_dev, H, W, radius, ctx->stream);
  DBM_API_END
}

int dbm_grid_to_pixel(dbm_ctx* ctx, const float* in_dev, long H, long W, double threshold, float* out_dev) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && in_dev != nullptr && out_dev != nullptr, "dbm_grid_to_pixel: NULL argument");
  note_device_write(ctx);
  check_plane("dbm_grid_to_pixel", H, W, 2, "H W must stay below 2^31 nodes", "the grid needs at least 2 x 2 nodes");
  DBM_CHECK(threshold > 0.0 && threshold <= 1.0, "dbm_grid_to_pixel: threshold must lie in (0, 1]");
  DBM_CHECK((const void*)in_dev != (const void*)out_dev, "dbm_grid_to_pixel: the output must not be the input");
  launch_grid_to_pixel(in_dev, H, W, threshold, out_dev, ctx->stream);
  DBM_API_END
}

// ---- nodes inside a buffered polygon set (polygon.hip) ----
int dbm_grid_polygon_mask(dbm_ctx* ctx, const double* edges, size_t n_edges, long H, long W, const double geom[4], double buffer,
                          unsigned char* mask_dev, float* grid_dev, size_t workspace_limit, int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && geom != nullptr, "dbm_grid_polygon_mask: NULL context or geometry");
  note_device_write(ctx);
  check_plane("dbm_grid_polygon_mask", H, W, 1, "H W must stay below 2^31 nodes", "empty raster");
  DBM_CHECK(n_edges < ((size_t)1 << 31), "dbm_grid_polygon_mask: n_edges must stay below 2^31");
  check_geometry("dbm_grid_polygon_mask", geom, "the geometry must be finite with non-zero dx and dy");
  DBM_CHECK(std::isfinite(buffer), "dbm_grid_polygon_mask: the buffer must be finite");
  DBM_CHECK(mask_dev != nullptr || grid_dev != nullptr, "dbm_grid_polygon_mask: both outputs are NULL");
  DBM_CHECK(n_edges == 0 || edges != nullptr, "dbm_grid_polygon_mask: NULL edge table");
  const bool dev = device_ptrs(flags);
  if (!dev)
    for (size_t i = 0; i < 4 * n_edges; ++i)
      DBM_CHECK(std::isfinite(edges[i]), "dbm_grid_polygon_mask: edge " + std::to_string(i / 4) + " has a non-finite coordinate");
  PolyLaunch a;
  a.n = (long)n_edges;
  a.H = H; a.W = W;
  a.x0 = geom[0]; a.y0 = geom[1]; a.dx = geom[2]; a.dy = geom[3];
  a.buffer = buffer;
  polygon_geometry(a);
  ScopedBuf ws, bins;   // this call's own, released on every path
  double* staged = polygon_carve(a, ws.as<char>(polygon_workspace(a, !dev)), !dev);
  a.edges = edges;
  if (!dev && n_edges > 0) {
    DBM_HIP(hipMemcpyAsync(staged, edges, n_edges * sizeof(double[4]), hipMemcpyHostToDevice, ctx->stream));
    a.edges = staged;
  }
  a.entries = nullptr;
  a.nP = a.nB = 0u;
  a.mask = mask_dev;
  a.grid = grid_dev;
  launch_polygon_cull(a, ctx->stream);
  unsigned long long totals[8];
  DBM_HIP(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  DBM_CHECK(totals[2] == 0ull, "dbm_grid_polygon_mask: " + std::to_string(totals[2]) + " edges have a non-finite coordinate; nothing was written");
  if (totals[3] != 0ull) a.identity = 1;
  a.nP = (unsigned)totals[0];
  a.nB = (unsigned)totals[1];
  const unsigned long long entries = totals[4] + totals[5];
  const size_t limit = workspace_limit ? workspace_limit : DBM_POLY_WORKSPACE_DEFAULT;
  const bool binned = !a.identity && n_edges > 0 && entries < (1ull << 31) && entries * sizeof(unsigned) <= limit;
  if (binned) {
    a.entries = bins.as<unsigned>(entries > 0 ? (size_t)entries : 1);
    launch_polygon_bin(a, ctx->stream);
  }
  launch_polygon_classify(a, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
  const long long stats[6] = {(long long)totals[0], (long long)totals[1], (long long)totals[4], (long long)totals[5],
                              a.identity ? 2LL : (binned ? 1LL : 0LL), (long long)n_edges};
  memcpy(ctx->poly_stats, stats, sizeof(stats));
  DBM_API_END
}

int dbm_grid_polygon_stats(dbm_ctx* ctx, int64_t out[6]) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && out != nullptr, "dbm_grid_polygon_stats: NULL argument");
  for (int k = 0; k < 6; ++k) out[k] = (int64_t)ctx->poly_stats[k];
  DBM_API_END
}

// ---- vector layers on a resident image (overlay.hip) ----
int dbm_image_overlay(dbm_ctx* ctx, unsigned char* image_dev, long H, long W, int channels, const double geom[4], const double* prims,
                      size_t n, int kind, int stride, double size_px, const unsigned char rgba[4], int samples, size_t workspace_limit,
                      int flags) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && image_dev != nullptr && geom != nullptr && rgba != nullptr, "dbm_image_overlay: NULL context, image, geometry or colour");
  note_device_write(ctx);
  check_plane("dbm_image_overlay", H, W, 1, "H W must stay below 2^31 pixels", "empty image");
  DBM_CHECK(channels == 3 || channels == 4, "dbm_image_overlay: channels must be 3 or 4");
  DBM_CHECK(n < ((size_t)1 << 31), "dbm_image_overlay: n must stay below 2^31");
  check_geometry("dbm_image_overlay", geom, "the geometry must be finite with non-zero dx and dy");
  DBM_CHECK(kind == DBM_OVERLAY_SEGMENTS || kind == DBM_OVERLAY_DISCS, "dbm_image_overlay: kind must be DBM_OVERLAY_SEGMENTS or DBM_OVERLAY_DISCS");
  DBM_CHECK(kind == DBM_OVERLAY_SEGMENTS ? stride == 4 : (stride == 2 || stride == 3),
            "dbm_image_overlay: the stride is 4 doubles for segments, 2 or 3 for discs");
  DBM_CHECK(std::isfinite(size_px) && size_px >= 0.0, "dbm_image_overlay: the size must be finite and not negative");
  DBM_CHECK(samples == 1 || samples == 2 || samples == 4, "dbm_image_overlay: samples must be 1, 2 or 4");
  DBM_CHECK(n == 0 || prims != nullptr, "dbm_image_overlay: NULL primitive table");
  const bool dev = device_ptrs(flags);
  const int used = kind == DBM_OVERLAY_SEGMENTS ? 4 : 2;   // columns that are coordinates
  if (!dev)
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < used; ++k)
        DBM_CHECK(std::isfinite(prims[i * (size_t)stride + k]), "dbm_image_overlay: primitive " + std::to_string(i) + " has a non-finite coordinate");
  OverlayLaunch a = {};
  a.n = (long)n;
  a.H = H; a.W = W;
  a.kind = kind; a.stride = stride; a.channels = channels; a.S = samples;
  a.x0 = geom[0]; a.y0 = geom[1]; a.dx = geom[2]; a.dy = geom[3];
  a.size = size_px;
  overlay_geometry(a);
  a.image = image_dev;
  memcpy(a.rgba, rgba, 4);
  a.word_aligned = ((uintptr_t)image_dev & 3u) == 0 ? 1 : 0;
  long long stats[4] = {0, 0, 0, (long long)n};
  if (n > 0) {
    ScopedBuf ws, bins;   // this call's own, released on every path
    double* staged = overlay_carve(a, ws.as<char>(overlay_workspace(a, !dev)), !dev);
    a.prims = prims;
    if (!dev) {
      DBM_HIP(hipMemcpyAsync(staged, prims, n * (size_t)stride * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      a.prims = staged;
    }
    launch_overlay_cull(a, ctx->stream);
    unsigned long long totals[8];
    DBM_HIP(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
    DBM_HIP(hipStreamSynchronize(ctx->stream));
    DBM_CHECK(totals[2] == 0ull, "dbm_image_overlay: " + std::to_string(totals[2]) + " primitives have a non-finite coordinate; nothing was written");
    a.kept = (unsigned)totals[0];
    const unsigned long long entries = totals[1];
    const size_t limit = workspace_limit ? workspace_limit : DBM_POLY_WORKSPACE_DEFAULT;
    const bool binned = a.kept > 0u && entries < (1ull << 31) && entries * sizeof(unsigned) <= limit;
    if (a.kept > 0u) {
      if (binned) {
        a.entries = bins.as<unsigned>((size_t)entries);
        launch_overlay_bin(a, ctx->stream);
      }
      launch_overlay_paint(a, ctx->stream);
    }
    DBM_HIP(hipStreamSynchronize(ctx->stream));   // the workspace is freed when this scope ends
    stats[0] = (long long)totals[0];
    stats[1] = (long long)totals[1];
    stats[2] = binned ? 1LL : 0LL;
  }
  memcpy(ctx->overlay_stats, stats, sizeof(stats));
  DBM_API_END
}

int dbm_image_overlay_stats(dbm_ctx* ctx, int64_t out[4]) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(ctx != nullptr && out != nullptr, "dbm_image_overlay_stats: NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = (int64_t)ctx->overlay_stats[k];
  DBM_API_END
}

}  // extern "C"
