// extern "C" surface of libdbm.so (include/dbm.h), op level: the dbm_op_* entry points, through which the op-level tests reach single
// launches as the models make them.  What they keep from call to call lives in the context (dbm_ctx::op).  (Training: api.hip; data
// preparation: api_data.hip.)
#include "api_common.h"

// a throw-away single-layer "model" whose param arena holds a copy of the caller's weights, and of the bias b where that is not null
static IgLayer make_temp_layer(dbm_ctx* ctx, dbm_model& holder, const float* w, const float* b, int O, int C, int k, int stride, int pad,
                               bool bias = true, bool as_1x1 = false) {
  holder.ctx = ctx;
  holder.add_tensor("op/W", {O, C, k, k}, DBM_KIND_PARAM);
  holder.add_tensor("op/b", {O}, DBM_KIND_PARAM);
  holder.alloc_arenas();
  DBM_HIP(hipMemcpyAsync(holder.params, w, sizeof(float) * (size_t)O * C * k * k, hipMemcpyDeviceToDevice, ctx->stream));
  holder.add_iglayer("op", O, C, k, stride, pad, bias, as_1x1);
  holder.ensure_packed();
  const IgLayer L = holder.layers[0];
  if (b) DBM_HIP(hipMemcpyAsync(holder.P(L.bi), b, sizeof(float) * O, hipMemcpyDeviceToDevice, ctx->stream));
  return L;
}

// a throw-away model that holds nothing but the generator's input block
static InputBlockIds make_temp_input_block(dbm_ctx* ctx, dbm_model& holder) {
  holder.ctx = ctx;
  const InputBlockIds ib = add_input_block(holder, "op/");
  holder.alloc_arenas();
  return ib;
}
// The block's eight tensors, (W, b) per convolution: from `in` into the holder's arena, or (in == null) from the arena to `out`; the
// parameter arena, or the gradient arena.
static void copy_input_block(const dbm_model& holder, const InputBlockIds& ib, bool grads, const float* const* in, float* const* out,
                             hipStream_t s) {
  for (int i = 0; i < 8; ++i) {
    const int t = ib.T[i / 2][i % 2];
    float* h = grads ? holder.G(t) : holder.P(t);
    DBM_HIP(hipMemcpyAsync(in ? h : out[i], in ? in[i] : h, sizeof(float) * holder.tensors[t].n, hipMemcpyDeviceToDevice, s));
  }
}

extern "C" {

int dbm_op_conv2d(dbm_ctx* ctx, const float* x, const float* w, const float* b, float* y, int N, int C, int H, int W,
                  int O, int k, int stride, int pad, int ups, int lrelu) {
  DBM_API_BEGIN(ctx)
  if (C % 32 != 0) {
    DBM_CHECK(!ups, "few-channel conv has no fused upsample");
    SmallConvDesc d = small_conv_desc(x, (long)C * H * W, C, H, W, O, k, stride, pad, N);
    d.w = w; d.bias = b; d.y = y; d.ysn = (long)O * d.OH * d.OW; d.act = lrelu; d.slope = 0.2f;
    launch_smallcin_conv_fwd(d, ctx->stream);
  } else {
    dbm_model holder;
    IgLayer L = make_temp_layer(ctx, holder, w, b, O, C, k, stride, pad);
    const int OH = conv_out_extent(H << ups, k, stride, pad), OW = conv_out_extent(W << ups, k, stride, pad);
    ConvDesc d = holder.fwd_desc(L, x, (long)C * H * W, H, W, ups, y, (long)O * OH * OW, N);
    d.act = lrelu;
    launch_igemm_conv(d, ctx->stream);
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  DBM_API_END
}

int dbm_op_conv2d_backward(dbm_ctx* ctx, const float* x, const float* w, const float* gy, float* gx, float* gw,
                           float* gb, int N, int C, int H, int W, int O, int k, int stride, int pad, int ups) {
  DBM_API_BEGIN(ctx)
  const int Hl = H << ups, Wl = W << ups;
  const int OH = conv_out_extent(Hl, k, stride, pad), OW = conv_out_extent(Wl, k, stride, pad);
  if (C % 32 != 0) {
    DBM_CHECK(!ups && gx == nullptr, "few-channel conv: only the weight gradient exists on the hot path");
    launch_smallcin_conv_wgrad(small_conv_desc(x, (long)C * H * W, C, H, W, O, k, stride, pad, N), gy, (long)O * OH * OW, gw, gb, ctx->stream);
  } else {
    DBM_CHECK(O % 32 == 0 || gx == nullptr, "op dgrad needs O % 32 == 0 (pad the gradient channels)");
    dbm_model holder;
    IgLayer L = make_temp_layer(ctx, holder, w, nullptr, O, C, k, stride, pad);
    if (gw)
      launch_wgrad(wgrad_desc(x, (long)C * H * W, C, H, W, ups, gy, (long)O * OH * OW, O, OH, OW, k, stride, pad, N, 1.f, gw, gb), ctx->stream);
    if (gx) {
      holder.ensure_packed_bwd();
      holder.run_dgrad(L, dbm_model::dgrad_desc(gy, (long)O * OH * OW, gx, (long)C * Hl * Wl, N), Hl, Wl);  // gradient w.r.t. the (upsampled) conv input
    }
    DBM_HIP(hipStreamSynchronize(ctx->stream));
  }
  DBM_API_END
}

// One forward or data-gradient launch exactly as the models make it: fwd_desc / dgrad_desc + run_dgrad, every epilogue field, strided
// operands; the launcher's choice comes back in `report` (include/dbm.h).
int dbm_op_conv2d_launch(dbm_ctx* ctx, const dbm_conv_launch* a, int* report) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(a != nullptr && a->x && a->y && a->w, "conv launch op: x, y and w are required");
  DBM_CHECK(a->C % 32 == 0 && a->C >= 32, "conv launch op: C must be a multiple of 32 (the implicit-GEMM kernels)");
  DBM_CHECK(a->N >= 1 && a->O >= 1 && a->H >= 1 && a->W >= 1 && (a->ups == 0 || a->ups == 1), "conv launch op: bad geometry");
  const int Cout = a->dgrad ? a->C : a->O;
  DBM_CHECK(!a->r1 || (a->r1_nch >= 0 && a->r1_nch <= Cout), "conv launch op: r1_nch outside the output channels");
  DBM_CHECK(!a->mask || (a->mask_c0 >= 0 && a->mask_c0 <= Cout), "conv launch op: mask_c0 outside the output channels");
  dbm_model holder;
  const bool has_bias = !a->dgrad && a->bias != nullptr;
  IgLayer L = make_temp_layer(ctx, holder, a->w, has_bias ? a->bias : nullptr, a->O, a->C, a->k, a->stride, a->pad, has_bias);
  auto epilogue = [&](ConvDesc& d) {
    d.act = a->act; d.s1 = a->s1;
    d.r1 = a->r1; d.r1sn = a->r1sn; d.r1_nch = a->r1_nch; d.r1s = a->r1s;
    d.r2 = a->r2; d.r2sn = a->r2sn; d.s2 = a->s2;
    d.accumulate = a->accumulate;
    d.mask = a->mask; d.masksn = a->masksn; d.mask_c0 = a->mask_c0;
    d.ch_scale = a->ch_scale;
  };
  std::vector<ConvLaunchReport> reps;
  if (!a->dgrad) {
    ConvDesc d = holder.fwd_desc(L, a->x, a->xsn, a->H, a->W, a->ups, a->y, a->ysn, a->N);
    epilogue(d);
    d.yt = a->yt;
    if (d.yt && !conv_tile_writes_yt(d)) d.yt = nullptr;   // (as Generator::forward asks before it hands the twin out)
    ConvLaunchReport r;
    launch_igemm_conv(d, ctx->stream, &r);
    reps.push_back(r);
  } else {
    DBM_CHECK(a->ups == 0 && a->bias == nullptr && a->ch_scale == nullptr && a->yt == nullptr,
              "conv launch op: a data gradient has no folded resize, bias, channel scale or channels-last twin");
    holder.ensure_packed_bwd();
    ConvDesc d = dbm_model::dgrad_desc(a->x, a->xsn, a->y, a->ysn, a->N);
    epilogue(d);
    holder.run_dgrad(L, d, a->H, a->W, nullptr, &reps);
  }
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  if (report) {
    report[0] = (int)reps.size();
    for (size_t i = 0; i < reps.size() && i < 4; ++i) {
      const ConvLaunchReport& r = reps[i];
      const int v[10] = {r.family, r.cfg, r.waves, r.npb, r.row, r.ksplit, r.nosplit, r.nphase, r.mt2, r.yt};
      memcpy(report + 1 + 10 * i, v, sizeof(v));
    }
  }
  DBM_API_END
}

// L weight gradients as ONE WgradBatch (the training step's form).  The context keeps the batch between calls with the same
// descriptors, as the step keeps its batches between iterations: a call that only switches the mode goes through WgradBatch::launch's
// re-plan.
int dbm_op_conv2d_wgrad_batch(dbm_ctx* ctx, const dbm_wgrad_desc* descs, int L, int cleared_target, int* cat_out, int* S_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(descs != nullptr && L >= 1, "wgrad batch op: no descriptors");
  WgradBatch& batch = ctx->op.wgrad_batch;
  std::vector<dbm_wgrad_desc>& key = ctx->op.wgrad_key;
  if ((int)key.size() != L || memcmp(key.data(), descs, sizeof(dbm_wgrad_desc) * (size_t)L) != 0) {
    batch.reset();
    key.assign(descs, descs + L);
    for (int i = 0; i < L; ++i) {
      const dbm_wgrad_desc& q = descs[i];
      // (C % 4: a ragged last input tile, e.g. 36 channels, as far as the 16-byte staging of the LDS-DMA forms takes one)
      DBM_CHECK(q.x && q.dy && q.gW && q.C % 4 == 0 && q.C >= 32 && q.N >= 1 && (q.ups == 0 || q.ups == 1),
                "wgrad batch op: x, dy, gW are required; C must be a multiple of 4, at least 32");
      const int OH = conv_out_extent(q.H << q.ups, q.k, q.stride, q.pad), OW = conv_out_extent(q.W << q.ups, q.k, q.stride, q.pad);
      DBM_CHECK(OH >= 1 && OW >= 1, "wgrad batch op: empty output plane");
      batch.add(wgrad_desc(q.x, q.xsn, q.C, q.H, q.W, q.ups, q.dy, q.dysn, q.O, OH, OW, q.k, q.stride, q.pad, q.N, q.scale, q.gW, q.gb));
    }
  }
  batch.cleared_target = cleared_target != 0;
  batch.launch(ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < L; ++i) {
    if (cat_out) cat_out[i] = batch.desc_cat[i];
    if (S_out) S_out[i] = batch.desc_S[i];
  }
  DBM_API_END
}

}  // extern "C"

// ---- the persistent trunk kernels at op level (include/dbm.h) ----
static const int TRUNK_PLANE = 81;
static const float TRUNK_SLOPE = 0.2f;

// the context's inbox for both ops (dbm_ctx::OpState), zeroed when it is made
static unsigned long long* op_trunk_inbox(dbm_ctx* ctx) {
  if (!ctx->op.trunk_inbox) {
    DBM_HIP(hipMalloc((void**)&ctx->op.trunk_inbox, trunk_fused_inbox_bytes(64)));
    DBM_HIP(hipMemset(ctx->op.trunk_inbox, 0, trunk_fused_inbox_bytes(64)));
    DBM_HIP(hipDeviceSynchronize());
  }
  return ctx->op.trunk_inbox;
}

// floats of dense block layer k's (0..4) OIHW weight tensor / bias
static size_t trunk_w_floats(int k) { return (size_t)(k < 4 ? 32 : 64) * (64 + 32 * k) * 9; }
static size_t trunk_b_floats(int k) { return k < 4 ? 32 : 64; }

// the nrdb * 5 host tensors of `host` (sizes by layer) into one device arena; their device addresses as a device table
static const float** upload_trunk_tensors(dbm_ctx* ctx, const float* const* host, int nrdb, bool bias, ScopedBuf& arena, ScopedBuf& table) {
  size_t total = 0;
  for (int i = 0; i < nrdb * 5; ++i) total += bias ? trunk_b_floats(i % 5) : trunk_w_floats(i % 5);
  arena.ensure(total);
  std::vector<const float*> ptrs(nrdb * 5);
  size_t off = 0;
  for (int i = 0; i < nrdb * 5; ++i) {
    const size_t n = bias ? trunk_b_floats(i % 5) : trunk_w_floats(i % 5);
    DBM_CHECK(host[i] != nullptr, "trunk op: a weight / bias pointer is null");
    DBM_HIP(hipMemcpyAsync(arena.p + off, host[i], n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ptrs[i] = arena.p + off;
    off += n;
  }
  const float** d = table.as<const float*>(ptrs.size());
  DBM_HIP(hipMemcpyAsync((void*)d, ptrs.data(), ptrs.size() * sizeof(float*), hipMemcpyHostToDevice, ctx->stream));
  DBM_HIP(hipStreamSynchronize(ctx->stream));  // (ptrs is a local)
  return d;
}

static void check_trunk_op(const dbm_ctx* ctx, int nrdb, int N, int ipl, int only_launch) {
  DBM_CHECK(nrdb >= 3 && nrdb % 3 == 0, "trunk op: nrdb must be a positive multiple of 3");
  DBM_CHECK(nrdb + 1 <= TRUNK_FUSED_MAXCAT, "trunk op: too many dense blocks for the persistent kernels");
  DBM_CHECK(N >= 1 && ipl >= 1 && ipl <= ctx->trunk_imgs, "trunk op: imgs_per_launch outside 1 .. the context's images per persistent launch");
  DBM_CHECK(only_launch < (N + ipl - 1) / ipl, "trunk op: only_launch past the last launch");
}

// The launch loop of both ops (Generator::forward's / ::backward's): `groups` passes from the top down, image chunks of IMGS inside,
// only chunk only_launch where that is >= 0.  The context's launch counter goes on, or restarts at epoch0 >= 0; every launch stands in
// the persist bracket.  fire(group, first image, images, epoch, report) fills and fires the op's own launch struct.
template <class Fire>
static std::vector<TrunkLaunchReport> run_trunk_launches(dbm_ctx* ctx, int groups, int N, int IMGS, int only_launch, int epoch0, Fire fire) {
  std::vector<TrunkLaunchReport> reps;
  int epoch = epoch0 >= 0 ? epoch0 - 1 : ctx->op.trunk_epoch;
  for (int g = 0; g < groups; ++g) {
    for (int i0 = 0; i0 < N; i0 += IMGS) {
      if (only_launch >= 0 && i0 / IMGS != only_launch) continue;
      TrunkLaunchReport r;
      ctx->persist_begin(ctx->stream);
      fire(g, i0, std::min(IMGS, N - i0), ++epoch, &r);
      ctx->persist_end(ctx->stream);
      reps.push_back(r);
    }
  }
  ctx->op.trunk_epoch = epoch;
  return reps;
}

// after the synchronisation: a bounded spin that ran out fails the call (the word is lowered again: no model is involved)
static void finish_trunk_op(dbm_ctx* ctx, const std::vector<TrunkLaunchReport>& reps, int* report, int report_cap) {
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  const bool gave_up = ctx->dev_err && *(volatile int*)ctx->dev_err;
  if (gave_up) {
    *(volatile int*)ctx->dev_err = 0;
    if (ctx->dev_err_flag) DBM_HIP(hipMemset(ctx->dev_err_flag, 0, sizeof(int)));
    DBM_HIP(hipDeviceSynchronize());
  }
  if (report && report_cap >= 1) {
    report[0] = (int)reps.size();
    for (size_t i = 0; i < reps.size() && 2 + 2 * (int)i < report_cap; ++i) {
      report[1 + 2 * i] = reps[i].form;
      report[2 + 2 * i] = reps[i].grid;
    }
  }
  if (gave_up) throw DbmError(7, "trunk op: a persistent kernel gave up waiting for a neighbouring workgroup");
}

extern "C" {

int dbm_op_trunk_forward(dbm_ctx* ctx, const dbm_trunk_forward* a, int* report, int report_cap) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(a != nullptr && a->w && a->b && a->cat && a->cat[0], "trunk forward op: w, b and cat[0] are required");
  check_trunk_op(ctx, a->nrdb, a->N, a->imgs_per_launch, a->only_launch);
  DBM_CHECK(a->tile == 27 || a->tile == 32, "trunk forward op: tile must be 27 or 32");
  DBM_CHECK(!a->helper || a->tile == 27, "trunk forward op: the helper form has 27-position tiles");
  DBM_CHECK(a->keep || a->out, "trunk forward op: out is required without keep");
  const int nrdb = a->nrdb, N = a->N, nbuf = a->keep ? nrdb + 1 : 2;
  const size_t catn = (size_t)N * 192 * TRUNK_PLANE;
  std::vector<float*> host(nbuf);
  for (int i = 0; i < nbuf; ++i) {
    host[i] = a->keep ? a->cat[i] : (i == 0 ? a->cat[0] : a->out);
    DBM_CHECK(host[i] != nullptr, "trunk forward op: a concat buffer is null");
  }
  ScopedBuf warena, barena, wtab, btab, wstream, bstream, bufs;
  const float** d_w = upload_trunk_tensors(ctx, a->w, nrdb, false, warena, wtab);
  const float** d_b = upload_trunk_tensors(ctx, a->b, nrdb, true, barena, btab);
  wstream.ensure(trunk_fused_stream_floats(nrdb));   // (zeroed: the read-ahead pad behind the last block)
  bstream.ensure((size_t)nrdb * 192);
  launch_pack_trunk_fused(d_w, d_b, wstream.p, bstream.p, nrdb, ctx->stream);
  bufs.ensure(catn * nbuf);
  std::vector<float*> dev(nbuf);
  for (int i = 0; i < nbuf; ++i) {
    dev[i] = bufs.p + catn * i;
    DBM_HIP(hipMemcpyAsync(dev[i], host[i], catn * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  unsigned long long* inbox = op_trunk_inbox(ctx);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  const std::vector<TrunkLaunchReport> reps = run_trunk_launches(
      ctx, 1, N, a->imgs_per_launch, a->only_launch, a->epoch0, [&](int, int i0, int nimg, int epoch, TrunkLaunchReport* r) {
        TrunkFusedLaunch L;
        L.wstream = wstream.p; L.bstream = bstream.p; L.in = dev[0];
        L.cat = a->keep ? dev.data() : nullptr; L.out = a->keep ? dev[nrdb] : dev[1];
        L.inbox = inbox; L.err = ctx->dev_err_d; L.err_dev = ctx->dev_err_flag;
        L.nrdb = nrdb; L.nimg = nimg; L.img0 = i0; L.epoch = epoch;
        L.rs = a->rs; L.slope = TRUNK_SLOPE;
        L.tile = a->tile; L.helper = a->helper ? 1 : 0; L.local_st = a->agent_stores ? 0 : 1;
        launch_trunk_fused(L, ctx->stream, r);
      });
  for (int i = 0; i < nbuf; ++i) DBM_HIP(hipMemcpyAsync(host[i], dev[i], catn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  finish_trunk_op(ctx, reps, report, report_cap);
  DBM_API_END
}

int dbm_op_trunk_backward(dbm_ctx* ctx, const dbm_trunk_backward* a, int* report, int report_cap) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(a != nullptr && a->w && a->cat && a->dA && a->gin && a->g_a3 && a->j0 && a->j1, "trunk backward op: a required pointer is null");
  check_trunk_op(ctx, a->nrdb, a->N, a->imgs_per_launch, a->only_launch);
  const int nrdb = a->nrdb, N = a->N;
  DBM_CHECK(a->gin_sn == 64 * TRUNK_PLANE || a->gin_sn == 192 * TRUNK_PLANE, "trunk backward op: gin's image stride is 64 * 81 or 192 * 81");
  DBM_CHECK(a->nlaunch >= 1, "trunk backward op: no launches");
  for (int i = 0; i < a->nlaunch; ++i) {
    DBM_CHECK(a->j0[i] >= 0 && a->j0[i] % 3 == 0 && a->j1[i] % 3 == 0 && a->j0[i] < a->j1[i] && a->j1[i] <= nrdb,
              "trunk backward op: launches cover whole RRDBs");
    DBM_CHECK(i == 0 || a->j1[i] == a->j0[i - 1], "trunk backward op: a launch starts where the one before ended");
  }
  const size_t catn = (size_t)N * 192 * TRUNK_PLANE;
  ScopedBuf warena, wtab, wstream, bufs, gin, ga3;
  const float** d_w = upload_trunk_tensors(ctx, a->w, nrdb, false, warena, wtab);
  wstream.ensure(trunk_fused_bwd_stream_floats(nrdb));
  launch_pack_trunk_fused_bwd(d_w, wstream.p, nrdb, ctx->stream);
  bufs.ensure(catn * 2 * nrdb);
  gin.ensure((size_t)N * a->gin_sn);
  ga3.ensure((size_t)N * 64 * TRUNK_PLANE);
  std::vector<float*> dAp(nrdb);
  std::vector<const float*> catp(nrdb);
  for (int j = 0; j < nrdb; ++j) {
    DBM_CHECK(a->cat[j] && a->dA[j], "trunk backward op: a concat buffer is null");
    float* c = bufs.p + catn * j;
    dAp[j] = bufs.p + catn * (nrdb + j);
    catp[j] = c;
    DBM_HIP(hipMemcpyAsync(c, a->cat[j], catn * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    DBM_HIP(hipMemcpyAsync(dAp[j], a->dA[j], catn * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  DBM_HIP(hipMemcpyAsync(gin.p, a->gin, (size_t)N * a->gin_sn * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  DBM_HIP(hipMemcpyAsync(ga3.p, a->g_a3, (size_t)N * 64 * TRUNK_PLANE * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  unsigned long long* inbox = op_trunk_inbox(ctx);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  const std::vector<TrunkLaunchReport> reps = run_trunk_launches(
      ctx, a->nlaunch, N, a->imgs_per_launch, a->only_launch, a->epoch0, [&](int g, int i0, int nimg, int epoch, TrunkLaunchReport* r) {
        TrunkFusedBwdLaunch L;
        L.wstream = wstream.p;
        L.gin = g == 0 ? gin.p : dAp[a->j1[g]]; L.gin_sn = g == 0 ? (long)a->gin_sn : 192L * TRUNK_PLANE;
        L.dA = dAp.data(); L.cat = catp.data(); L.g_a3 = ga3.p;
        L.inbox = inbox; L.err = ctx->dev_err_d; L.err_dev = ctx->dev_err_flag;
        L.nrdb = nrdb; L.j0 = a->j0[g]; L.j1 = a->j1[g]; L.nimg = nimg; L.img0 = i0; L.epoch = epoch;
        L.rs = a->rs; L.slope = TRUNK_SLOPE;
        L.local_st = a->agent_stores ? 0 : 1;
        launch_trunk_fused_bwd(L, ctx->stream, r);
      });
  for (int j = 0; j < nrdb; ++j) DBM_HIP(hipMemcpyAsync(a->dA[j], dAp[j], catn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  finish_trunk_op(ctx, reps, report, report_cap);
  DBM_API_END
}

// 3x3 / stride 1 / pad 1 convolution through the channels-last bf16 kernel of the sweep's trunk (conv_cl16.hip), for the parity
// tests: x (N, C, H, W) fp32 is rounded to bf16 NHWC, y = [lrelu](s1 * (conv + b) + r1), fp32 out.  All DEVICE pointers.
int dbm_op_conv2d_cl16(dbm_ctx* ctx, const float* x, const float* w, const float* b, const float* r1, float s1, float* y, int N,
                       int C, int H, int W, int O, int lrelu) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(C % 32 == 0 && C >= 32 && C <= 256 && (O == 32 || O == 64), "cl16 conv op: C % 32 == 0, O 32 or 64");
  DBM_CHECK(r1 == nullptr || O == 64, "cl16 conv op: the residual input has 64 channels");
  hipStream_t s = ctx->stream;
  const int plane = H * W;
  const size_t P = (size_t)N * plane;
  ScopedBuf act, res, out, wimg, bias;
  act.ensure(P * C / 2 + 8);
  out.ensure(P * 64);
  wimg.ensure(cl16_packed_elems(C, O) / 2 + 8);
  bias.ensure(64);
  if (b) DBM_HIP(hipMemcpyAsync(bias.p, b, sizeof(float) * O, hipMemcpyDeviceToDevice, s));
  for (int c0 = 0; c0 < C; c0 += 64)
    launch_nchw_to_cl(x + (size_t)c0 * plane, (long)C * plane, nullptr, (char*)act.p + 2 * (size_t)c0, C, N, plane, s, std::min(64, C - c0));
  if (r1) {
    res.ensure(P * 64);
    launch_nchw_to_cl(r1, 64L * plane, res.p, nullptr, 0, N, plane, s);
  }
  launch_pack_cl16(w, wimg.p, O, C, s);
  ClConvLaunch q;
  memset(&q, 0, sizeof(q));
  q.x = act.p; q.xc = C; q.Cin = C; q.Cout = O; q.w = wimg.p; q.bias = bias.p; q.y32 = out.p;
  q.r1 = r1 ? res.p : nullptr; q.s1 = r1 ? s1 : 1.f; q.s2 = 1.f; q.act = lrelu; q.slope = 0.2f; q.N = N; q.H = H; q.W = W;
  q.zeros = ctx->zeros;
  launch_conv_cl16(q, s);
  launch_cl_to_nchw(out.p, y, (long)O * plane, N, plane, s, O);
  DBM_HIP(hipStreamSynchronize(s));
  DBM_API_END
}

// The split-bf16 form (conv_cl16x3_kernel: three bf16 MFMAs per product) of the same convolution, optionally on the nearest x2
// resize of x: x (N, 64, H >> ups, W >> ups), y (N, O, H, W), O <= 64; planar != 0 writes y through the kernel's channel-plane
// epilogue (the offset tensors' form) instead of NHWC + transpose.  All DEVICE pointers.
int dbm_op_conv2d_cl16x3(dbm_ctx* ctx, const float* x, const float* w, const float* b, float* y, int N, int H, int W, int O, int ups,
                         int lrelu, int planar) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(O >= 1 && O <= 64 && (ups == 0 || ups == 1), "cl16x3 conv op: O <= 64, ups 0 / 1");
  hipStream_t s = ctx->stream;
  const int Hs = H >> ups, Ws = W >> ups, plane = H * W, splane = Hs * Ws;
  ScopedBuf xin, out, wimg, bias;
  xin.ensure((size_t)N * splane * 64);
  out.ensure((size_t)N * plane * 64);
  wimg.ensure(cl16x3_packed_elems(64, O) / 2 + 8);
  bias.ensure(64);
  if (b) DBM_HIP(hipMemcpyAsync(bias.p, b, sizeof(float) * O, hipMemcpyDeviceToDevice, s));
  launch_nchw_to_cl(x, 64L * splane, xin.p, nullptr, 0, N, splane, s);
  launch_pack_cl16x3(w, wimg.p, O, 64, s);
  ClX3Launch q;
  memset(&q, 0, sizeof(q));
  q.x = xin.p; q.xc = 64; q.Cin = 64; q.Cout = O; q.ups = ups; q.w = wimg.p; q.bias = bias.p; q.act = lrelu; q.slope = 0.2f;
  q.N = N; q.H = H; q.W = W;
  if (planar) {
    DBM_HIP(hipMemsetAsync(y, 0, sizeof(float) * (size_t)N * O * plane, s));
    q.yp = y; q.ysn = (long)O * plane; q.ypc = O;
  } else {
    q.y32 = out.p; q.yc = 64;
  }
  launch_conv_cl16x3(q, s);
  if (!planar) launch_cl_to_nchw(out.p, y, (long)O * plane, N, plane, s, O);
  DBM_HIP(hipStreamSynchronize(s));
  DBM_API_END
}

// One named forward form of a deformable layer, whatever the switches say (the parity tests of the forms against each other).
int dbm_op_deform_conv2d_form(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* b, float* y, int N, int H,
                              int W, int O, int form, int lrelu) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK((form == 1 && O >= 1 && O <= 16) || ((form == 2 || form == 3 || form == 4) && O == 64),
            "deform conv op: form 1 (O <= 16, premultiplied) or 2 (O = 64, split-bf16; 3: its LDS-window kernel, 4: its gathering kernel)");
  hipStream_t s = ctx->stream;
  const long plane = (long)H * W;
  ScopedBuf xt, z, wx;
  xt.ensure((size_t)N * 64 * plane);
  launch_nchw_to_nhwc64(x, xt.p, N, (int)plane, s);
  if (form == 1) {
    z.ensure((size_t)N * 9 * O * plane);
    launch_deform_conv_fused(xt.p, off, w, b, y, nullptr, nullptr, N, 64, H, W, 18L * plane, O, 0, 0.2f, s, z.p);
  } else {
    wx.ensure((deform_x3_packed_elems() + 1) / 2);
    launch_pack_deform_x3(w, wx.p, s);
    launch_deform_conv64_x3(xt.p, off, wx.p, b, y, nullptr, N, H, W, 18L * plane, lrelu, 0.2f, s, form == 3 ? 1 : form == 4 ? 0 : -1);
  }
  DBM_HIP(hipStreamSynchronize(s));
  DBM_API_END
}

// The two entry points below run the generator's own launch sequences (deform_layer.hip) on scoped temporaries: they size buffers,
// transpose, build the temporary layer and call; which kernel form runs is decided there.
int dbm_op_deform_conv2d(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* b, float* y,
                         int N, int C, int H, int W, int O) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(C % 32 == 0, "deform conv op: C % 32 == 0");
  hipStream_t s = ctx->stream;
  const long P = (long)H * W;
  const DeformForms f = deform_layer_forms(C, O, H, W);
  ScopedBuf col, xt;
  dbm_model holder;   // (stays empty where the form reads the OIHW tensor itself)
  if (f.fwd_fused) {
    xt.ensure((size_t)N * C * P);
    launch_nchw_to_nhwc64(x, xt.p, N, (int)P, s);
  } else {
    col.ensure((size_t)N * C * 9 * P);
  }
  const float* bias = b;
  if (f.fwd_packed) {
    const IgLayer L = make_temp_layer(ctx, holder, w, b, O, C, 3, 1, 0, true, /*as_1x1=*/true);
    if (b) bias = holder.P(L.bi);
  }
  // (the few-output-channel form reads the OIHW weights directly; without the z scratch: the gather-then-multiply kernel)
  deform_layer_forward(holder, f.fwd_packed ? &holder.layers[0] : nullptr, f, x, xt.p, off, 18 * P, w, bias, y, nullptr, col.p, nullptr, N, C, H, W,
                       O, 0, s);
  DBM_HIP(hipStreamSynchronize(s));
  DBM_API_END
}

// One deformable forward exactly as Generator::forward launches it: the offsets at their own image stride, the activation, the
// channels-last twin, the retained sample matrix and the retained premultiplied planes, each handed to the launcher as given (null
// stays null).  Form 0 is the layer's own choice (deform_layer_forms + deform_layer_forward on the packed temporary layer); the other
// forms name one launcher.  report[0] (HOST, may be NULL): the path taken (include/dbm.h); which kernel a launcher then chose shows
// in the profiler's tags.
int dbm_op_deform_forward_launch(dbm_ctx* ctx, const dbm_deform_launch* a, int* report) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(a != nullptr && a->x && a->off && a->w, "dbm_op_deform_forward_launch: x, off and w are required");
  DBM_CHECK(a->N >= 1 && a->H >= 1 && a->W >= 1 && a->O >= 1, "dbm_op_deform_forward_launch: bad geometry");
  DBM_CHECK(a->form >= 0 && a->form <= 6, "dbm_op_deform_forward_launch: form 0 .. 6");
  const int N = a->N, H = a->H, W = a->W, O = a->O, C = 64, form = a->form;
  const long P = (long)H * W;
  DBM_CHECK(a->offsn >= 18 * P, "dbm_op_deform_forward_launch: offsn below the 18 offset planes of an image");
  DBM_CHECK(a->act == 0 || a->act == 1, "dbm_op_deform_forward_launch: act is 0 or 1");
  hipStream_t s = ctx->stream;
  DeformForms f = deform_layer_forms(C, O, H, W);
  if (form == 6) f.fwd_fused = f.premul = false, f.fwd_packed = O != 1;
  const bool fused = form != 6 && (form != 0 || f.fwd_fused);
  const bool x3 = form >= 2 && form <= 4, few = fused && !x3 && O <= 16;
  int path;
  if (x3) {
    DBM_CHECK(O == 64, "dbm_op_deform_forward_launch: forms 2, 3, 4 (split-bf16) are the 64 -> 64 layer's");
    DBM_CHECK(!a->colout && !a->z, "dbm_op_deform_forward_launch: the split-bf16 kernels write neither a sample matrix nor premultiplied planes");
    path = 4;
  } else if (form == 1 || form == 5) {
    DBM_CHECK(O <= 16, "dbm_op_deform_forward_launch: forms 1 and 5 are the few-output-channel layer's (O <= 16)");
    DBM_CHECK(form == 1 || !a->z, "dbm_op_deform_forward_launch: form 5 (gather, then multiply) has no premultiplied planes");
    path = form == 1 ? 2 : 3;
  } else if (fused) {
    DBM_CHECK(deform_conv_fused_ok(C, O), "dbm_op_deform_forward_launch: the fused forms take 64 or <= 16 output channels");
    path = O == 64 ? 1 : f.premul ? 2 : 3;
  } else {
    DBM_CHECK(O == 1 || O % 32 == 0, "dbm_op_deform_forward_launch: the unfused path takes O == 1 (GEMV) or O % 32 == 0 (implicit GEMM)");
    DBM_CHECK(!a->z, "dbm_op_deform_forward_launch: the unfused path has no premultiplied planes");
    path = O == 1 ? 5 : 6;
  }
  if (few) {
    DBM_CHECK(!a->act, "dbm_op_deform_forward_launch: the few-output-channel kernels have no activation");
    DBM_CHECK(!a->colout, "dbm_op_deform_forward_launch: the few-output-channel kernels write no sample matrix");
  }
  if (path == 5) DBM_CHECK(!a->act, "dbm_op_deform_forward_launch: the GEMV has no activation");
  const bool twin_ok = fused && O == 64;
  DBM_CHECK(!a->yt || twin_ok, "dbm_op_deform_forward_launch: only the fused 64 -> 64 kernels write the channels-last twin");
  DBM_CHECK(a->y || (a->yt && twin_ok), "dbm_op_deform_forward_launch: y may be null only where yt is written");
  DBM_CHECK(!a->z || path == 2, "dbm_op_deform_forward_launch: z belongs to the premultiplied form");

  ScopedBuf xt, col, zs, wx;
  dbm_model holder;   // (stays empty where the form reads the OIHW tensor itself)
  if (fused) {
    xt.ensure((size_t)N * C * P);
    launch_nchw_to_nhwc64(a->x, xt.p, N, (int)P, s);
  }
  if (x3) {
    wx.ensure((deform_x3_packed_elems() + 1) / 2);
    launch_pack_deform_x3(a->w, wx.p, s);
    launch_deform_conv64_x3(xt.p, a->off, wx.p, a->bias, a->y, a->yt, N, H, W, a->offsn, a->act, 0.2f, s, form == 3 ? 1 : form == 4 ? 0 : -1);
  } else if (form == 1 || form == 5) {
    float* z = a->z;
    if (form == 1 && !z) {
      zs.ensure((size_t)N * 9 * O * P);
      z = zs.p;
    }
    launch_deform_conv_fused(xt.p, a->off, a->w, a->bias, a->y, nullptr, nullptr, N, C, H, W, a->offsn, O, 0, 0.2f, s, z);
  } else {
    const float* bias = a->bias;
    if (f.fwd_packed) {
      const IgLayer L = make_temp_layer(ctx, holder, a->w, a->bias, O, C, 3, 1, 0, true, /*as_1x1=*/true);
      if (a->bias) bias = holder.P(L.bi);
    }
    float* colp = a->colout;
    if (!fused && !colp) {   // (the unfused path's scratch, where the caller does not keep it)
      col.ensure((size_t)N * C * 9 * P);
      colp = col.p;
    }
    float* z = nullptr;
    if (f.premul) {   // (Generator::forward: ws.zdef whenever the layer premultiplies)
      z = a->z;
      if (!z) {
        zs.ensure((size_t)N * 9 * O * P);
        z = zs.p;
      }
    }
    deform_layer_forward(holder, f.fwd_packed ? &holder.layers[0] : nullptr, f, a->x, xt.p, a->off, a->offsn, a->w, bias, a->y, a->yt, colp, z, N,
                         C, H, W, O, a->act, s);
  }
  DBM_HIP(hipStreamSynchronize(s));
  if (report) report[0] = path;
  DBM_API_END
}

int dbm_op_deform_conv2d_backward(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* gy,
                                  float* gx, float* goff, float* gw, float* gb, int N, int C, int H, int W, int O) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(C % 32 == 0, "deform conv op: C % 32 == 0");
  DBM_CHECK(O == 1 || O % 32 == 0, "deform conv op backward: O == 1 or O % 32 == 0");
  hipStream_t s = ctx->stream;
  const long P = (long)H * W;
  const DeformForms f = deform_layer_forms(C, O, H, W);
  ScopedBuf col, gcol, xt, part, cws, z, gt;
  if (f.bwd_fused) {
    cws.ensure(deform_csr_workspace_floats(N, H, W));
    xt.ensure((size_t)N * C * P);
    launch_nchw_to_nhwc64(x, xt.p, N, (int)P, s);
  } else {
    cws.ensure(deform_backward_workspace_floats(N, C, H, W));
  }
  if (!(f.bwd_fused && O == 1)) {   // (what a retained forward leaves for the forms that read the sample matrix)
    col.ensure((size_t)N * C * 9 * P);
    launch_deform_sample(x, off, col.p, N, C, H, W, 18 * P, s);
  }
  if (O == 1) {
    if (f.bwd_fused) part.ensure(deform_bwd1_partial_floats(N, H, W));
    if (f.premul_bwd) {   // (... and its premultiplied planes)
      z.ensure((size_t)N * 9 * P);
      gt.ensure((size_t)N * 9 * P);
      launch_deform1_premul(xt.p, w, z.p, N, H, W, 1, s);
    }
    deform1_backward(f, x, xt.p, off, 18 * P, w, gy, z.p, col.p, gx, goff, gw, gb, part.p, cws.p, gt.p, false, N, C, H, W, s, s, s);
  } else {
    dbm_model holder;
    const IgLayer L = make_temp_layer(ctx, holder, w, nullptr, O, C, 3, 1, 0, true, /*as_1x1=*/true);
    holder.ensure_packed_bwd();
    gcol.ensure((size_t)N * C * 9 * P);
    deform64_backward_data(holder, L, f, x, xt.p, off, 18 * P, gy, gcol.p, gx, goff, cws.p, false, N, H, W, s);
    if (f.wgrad_fused) part.ensure(deform_wgrad64_partial_floats(N, H, W));
    deform64_wgrad(holder, L, f, xt.p, col.p, off, 18 * P, gy, gw, gb, part.p, N, H, W, s, nullptr);
  }
  DBM_HIP(hipStreamSynchronize(s));
  DBM_API_END
}

// Training-mode BatchNorm + LeakyReLU exactly as the discriminator launches it (discriminator.hip: eps 1e-5, decay 0.9, slope 0.2, the
// context's time-out word as `hold`): which of the six kernel forms runs is launch_bn_train_fwd's own choice, reported through form_out
// (a BnForm; -1 with sync: the sync_batch_stats kernels at world = 1, no all-reduce).
int dbm_op_batchnorm_train(dbm_ctx* ctx, const float* z, const float* gamma, const float* beta, float* avg_mean, float* avg_var, float* y,
                           float* mean, float* inv_std, int N, int C, int plane, int sync, int* form_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(N >= 1 && C >= 1 && plane >= 1, "batchnorm op: N, C, plane >= 1");
  hipStream_t s = ctx->stream;
  if (sync) {
    ScopedBuf buf;
    buf.ensure(3 * (size_t)C);
    launch_bn_sync_stats(z, buf.p, N, C, plane, s);
    launch_bn_sync_fwd_apply(z, y, gamma, beta, buf.p, mean, inv_std, avg_mean, avg_var, N, C, plane, 1, 1e-5f, 0.9f, 0.2f, s, ctx->dev_err_flag);
    DBM_HIP(hipStreamSynchronize(s));
  } else {
    launch_bn_train_fwd(z, y, gamma, beta, mean, inv_std, avg_mean, avg_var, N, C, plane, 1e-5f, 0.9f, 0.2f, s, ctx->dev_err_flag);
    DBM_HIP(hipStreamSynchronize(s));
  }
  if (form_out) *form_out = sync ? -1 : (int)bn_train_form(N, C, plane);
  DBM_API_END
}

int dbm_op_batchnorm_train_backward(dbm_ctx* ctx, const float* z, const float* gh, const float* gamma, const float* beta, const float* mean,
                                    const float* inv_std, float* gz, float* ggamma, float* gbeta, int N, int C, int plane, int sync,
                                    int* form_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(N >= 1 && C >= 1 && plane >= 1, "batchnorm op: N, C, plane >= 1");
  hipStream_t s = ctx->stream;
  if (sync) {
    ScopedBuf buf;
    buf.ensure(2 * (size_t)C);
    launch_bn_sync_bwd_sums(z, gh, gamma, beta, mean, inv_std, buf.p, ggamma, gbeta, N, C, plane, 0.2f, s);
    launch_bn_sync_bwd_apply(z, gh, gamma, beta, mean, inv_std, buf.p, gz, N, C, plane, 1, 0.2f, s);
    DBM_HIP(hipStreamSynchronize(s));
  } else {
    launch_bn_train_bwd(z, gh, gamma, beta, mean, inv_std, gz, ggamma, gbeta, nullptr, N, C, plane, 0.2f, s);
    DBM_HIP(hipStreamSynchronize(s));
  }
  if (form_out) *form_out = sync ? -1 : (int)bn_train_form(N, C, plane);
  DBM_API_END
}

// The discriminator's head, 512 -> 100 -> 1, through the launches Discriminator::forward / ::backward use.
int dbm_op_disc_head(dbm_ctx* ctx, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* l1,
                     float* logits, int N) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(N >= 1, "disc head op: N >= 1");
  launch_disc_head_fwd(x, W1, b1, W2, b2, l1, logits, N, 512, 100, 0.2f, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  DBM_API_END
}

int dbm_op_disc_head_backward(dbm_ctx* ctx, const float* x, const float* W1, const float* W2, const float* glogits, const float* l1, float* gx,
                              float* gW1, float* gb1, float* gW2, float* gb2, int N, int* fused_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(N >= 1, "disc head op: N >= 1");
  ScopedBuf g_l1;
  g_l1.ensure((size_t)N * 100);
  const bool fused = disc_head_backward(x, W1, W2, glogits, l1, g_l1.p, gx, gW1, gb1, gW2, gb2, N, 512, 100, 0.2f, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  if (fused_out) *fused_out = fused ? 1 : 0;
  DBM_API_END
}

// The two entry points below run the generator's own launch sequences of the input block (generator.hip) on a throw-away model that
// holds nothing but the block: they copy the caller's tensors in, size the im2col images and call; form choice and launches are there.
int dbm_op_input_block(dbm_ctx* ctx, const float* x, const float* w1, const float* w2, const float* w3, const float* wx, const float* bx,
                       const float* ww1, const float* b1, const float* ww2, const float* b2, const float* ww3, const float* b3, float* y,
                       int64_t ysn, float* yt, int N, int H, int W, int form, int* form_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(x && w1 && w2 && w3 && wx && bx && ww1 && b1 && ww2 && b2 && ww3 && b3 && y, "input block op: every input, weight, bias and y are required");
  DBM_CHECK(N >= 1 && H >= 3 && W >= 3, "input block op: N >= 1 and tiles of at least 3 x 3");
  DBM_CHECK(form >= -1 && form <= 2, "input block op: form is -1 (the model's choice), 0 (layer-wise), 1 (fused) or 2 (rows)");
  const long hw = (long)(H - 2) * (W - 2);
  DBM_CHECK(ysn >= 128 * hw, "input block op: ysn must be at least 128 * (H - 2) * (W - 2)");
  if (form == IN_FUSED) {
    DBM_CHECK(input_block_fused_ok(H, W), "input block op: form 1 (the fused kernel) serves 11 x 11 tiles only");
    DBM_CHECK((reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2)) % 16 == 0,
              "input block op: form 1 (the fused kernel) stages w1 / w2 with 16-byte loads, both must be 16-byte aligned");
  }
  if (form == IN_ROWS)
    DBM_CHECK(input_block_rows_ok(H, W), "input block op: form 2 (the rows kernel) needs H >= 3 and planes at least two tiles wide (W - 2 >= 64)");
  const InputBlockForm f = form < 0 ? input_block_form(H, W, w1, w2, false) : (InputBlockForm)form;
  DBM_CHECK(!yt || f == IN_ROWS, "input block op: yt (channels-last) is written by form 2 (the rows kernel) only");
  hipStream_t s = ctx->stream;
  dbm_model holder;
  const InputBlockIds ib = make_temp_input_block(ctx, holder);
  const float* src[8] = {wx, bx, ww1, b1, ww2, b2, ww3, b3};
  copy_input_block(holder, ib, /*grads=*/false, src, nullptr, s);
  holder.ensure_packed();
  ScopedBuf colW1, colW2;
  if (f == IN_LAYERWISE) {
    colW1.ensure((size_t)N * holder.layers[ib.L[1]].CinP * hw);
    colW2.ensure((size_t)N * holder.layers[ib.L[2]].CinP * hw);
  }
  input_block_forward(holder, ib, f, N, H, W, x, w1, w2, w3, y, ysn, yt, colW1.p, colW2.p, false, s);
  DBM_HIP(hipStreamSynchronize(s));
  if (form_out) *form_out = (int)f;
  DBM_API_END
}

int dbm_op_input_block_backward(dbm_ctx* ctx, const float* x, const float* w1, const float* w2, const float* w3, const float* g, int64_t gsn,
                                float* gwx, float* gbx, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3, int N, int H,
                                int W, int* cat_out, int* S_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(x && w1 && w2 && w3 && g && gwx && gbx && gw1 && gb1 && gw2 && gb2 && gw3 && gb3, "input block op: every input, g and gradient are required");
  DBM_CHECK(N >= 1 && H >= 3 && W >= 3, "input block op: N >= 1 and tiles of at least 3 x 3");
  const long hw = (long)(H - 2) * (W - 2);
  DBM_CHECK(gsn >= 128 * hw, "input block op: gsn must be at least 128 * (H - 2) * (W - 2)");
  hipStream_t s = ctx->stream;
  dbm_model holder;
  const InputBlockIds ib = make_temp_input_block(ctx, holder);
  // (the model's launches add into the model's own gradient arena: the caller's gradients go in first and come back with the sums on top)
  float* dst[8] = {gwx, gbx, gw1, gb1, gw2, gb2, gw3, gb3};
  copy_input_block(holder, ib, /*grads=*/true, dst, nullptr, s);
  ScopedBuf colW1, colW2;
  colW1.ensure((size_t)N * holder.layers[ib.L[1]].CinP * hw);
  colW2.ensure((size_t)N * holder.layers[ib.L[2]].CinP * hw);
  WgradBatch batch;
  input_block_queue_wgrads(holder, ib, N, H, W, colW1.p, colW2.p, g, gsn, &batch);
  ctx->fork_to_side(6);
  input_block_rebuild_cols(holder, ib, N, H, W, w1, w2, colW1.p, colW2.p, ctx->side);
  batch.launch(ctx->side);
  input_block_small_wgrads(holder, ib, N, H, W, x, w3, g, gsn, ctx->side);
  ctx->join_side();
  copy_input_block(holder, ib, /*grads=*/true, nullptr, dst, s);
  DBM_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 2; ++i) {
    if (cat_out) cat_out[i] = batch.desc_cat[i];
    if (S_out) S_out[i] = batch.desc_S[i];
  }
  DBM_API_END
}

int dbm_op_smallcin_wgrad(dbm_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int N, int C, int H, int W, int O, int k,
                          int stride, int pad, int with_scratch, int* form_out) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(x && gy && gw, "few-channel wgrad op: x, gy and gw are required");
  DBM_CHECK(N >= 1 && C >= 1 && O >= 1 && k >= 1 && stride >= 1 && pad >= 0 && H + 2 * pad >= k && W + 2 * pad >= k, "few-channel wgrad op: bad geometry");
  const int OH = conv_out_extent(H, k, stride, pad), OW = conv_out_extent(W, k, stride, pad);
  DBM_CHECK((long)N * OH * OW < (1L << 31), "few-channel wgrad op: the kernels count positions in 32 bits");
  ScopedBuf scratch;
  if (with_scratch) scratch.ensure(smallcin_wgrad_scratch_floats(O));   // (as Discriminator::backward sizes c0_scratch)
  int form = 0;
  launch_smallcin_conv_wgrad(small_conv_desc(x, (long)C * H * W, C, H, W, O, k, stride, pad, N), gy, (long)O * OH * OW, gw, gb, ctx->stream,
                             scratch.p, &form);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  if (form_out) *form_out = form;
  DBM_API_END
}

int dbm_op_sumpool2(dbm_ctx* ctx, const float* g, const float* mask, float* out, int64_t nc, int H, int W) {
  DBM_API_BEGIN(ctx)
  DBM_CHECK(g && out && nc >= 1 && H >= 1 && W >= 1, "sumpool2 op: g, out and a non-empty output are required");
  DBM_CHECK((nc * H * W + 255) / 256 < (1L << 31), "sumpool2 op: too many elements for one launch");
  launch_sumpool2(g, mask, out, (long)nc, H, W, 0.2f, ctx->stream);
  DBM_HIP(hipStreamSynchronize(ctx->stream));
  DBM_API_END
}

}  // extern "C"
