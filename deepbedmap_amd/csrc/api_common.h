// What the extern "C" translation units of libdbm.so share: the exception boundary and the few helpers their entry points have in
// common.  api.hip holds the training surface (contexts, models, losses, the optimizer, the fused steps), api_data.hip the
// data-preparation surface (dbm_grid_*, dbm_points_*, dbm_text_*, dbm_tiff_*, dbm_chunk_*), api_ops.hip the op-level one (dbm_op_*).
#pragma once
#include "model.h"
#include <cmath>

// api.hip: the message dbm_last_error returns -- for the calling thread, and for `ctx` unless it is null
void api_record_error(dbm_ctx* ctx, const char* what);

// No exception crosses the boundary: an entry point's body stands between these two.
#define DBM_API_BEGIN(ctxptr) \
  dbm_ctx* _ectx = (ctxptr);  \
  (void)_ectx;                \
  try {
#define DBM_API_END                      \
  return 0;                              \
  }                                      \
  catch (const DbmError& e) {            \
    api_record_error(_ectx, e.what());   \
    return e.code;                       \
  }                                      \
  catch (const std::exception& e) {      \
    api_record_error(_ectx, e.what());   \
    return 3;                            \
  }

// the array arguments of this call are device pointers: it only enqueues (host pointers: staged, and the call synchronises)
inline bool device_ptrs(int flags) { return (flags & DBM_DEVICE_PTRS) != 0; }

// caller-visible device memory changes: retained generator forwards keyed on it go stale (Generator::has_graph_of compares
// data_epoch).  The rule: an entry point that can write or free such memory calls this ONCE, at its head -- behind its null-context
// check, before the other argument checks, under its `dev` condition where only the device-pointer form writes -- so that no path
// enqueues a write first.  A call that is refused afterwards has only made a retained forward be recomputed.
inline void note_device_write(dbm_ctx* ctx) { ctx->data_epoch++; }

// g = {x0, y0, dx, dy, ...} of a raster; the wording of the message is the caller's
inline void check_geometry(const char* who, const double* g, const char* message = "x0, y0 finite, dx, dy finite and non-zero") {
  DBM_CHECK(std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]) && std::isfinite(g[3]) && g[2] != 0.0 && g[3] != 0.0,
            std::string(who) + ": " + message);
}

// a plane whose kernels index nodes with 32-bit integers: H, W >= lo, and H, W, H * W below 2^31 (a call that words the lower bound
// separately passes that message too)
inline void check_plane(const char* who, long H, long W, long lo, const char* message, const char* too_small = nullptr) {
  DBM_CHECK(H >= lo && W >= lo, std::string(who) + ": " + (too_small ? too_small : message));
  DBM_CHECK(H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31), std::string(who) + ": " + message);
}

// host form of a table argument: room for `count` doubles in ctx->stage[k] (never less than one, so the pointer is not null), and
// the table copied up on the stream; host == nullptr: a result table, only sized
inline double* stage_table(dbm_ctx* ctx, int k, const double* host, size_t count) {
  double* st = ctx->stage[k].as<double>(count > 0 ? count : 1);
  if (host && count > 0) DBM_HIP(hipMemcpyAsync(st, host, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return st;
}
