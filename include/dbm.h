/* libdbm.so -- C ABI of the MI355X-native (gfx950) ESRGAN hot path of weiji14/deepbedmap.
 *
 * The reference has no FFI of its own: the path sits behind Python classes/functions of
 * srgan_train.py that call Chainer.  Each entry point below names the reference interface
 * (file:line under the reference checkout) it stands in for; INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.  Conventions:
 *   - every function returns 0 on success, non-zero on error; dbm_last_error() gives the text;
 *     nothing throws across the boundary.  Status 7 is recoverable: a persistent kernel gave up waiting for a
 *     neighbouring workgroup (the GPU is shared or partitioned).  From that moment a sticky device flag turns every
 *     optimizer launch and every BatchNorm running-average write into a no-op, so no parameter, moment or running
 *     statistic absorbs the invalid pass.  The condition is observed ONLY at the entry of the step entry points
 *     (dbm_train_iteration, dbm_discriminator_step, dbm_generator_step, dbm_adam_update) and by dbm_check_timeout: the call
 *     drains the device, gives the skipped launches' step counts back, switches to the layer-by-layer trunk kernels for a
 *     while (re-armed after DBM_TRUNK_REARM = 64 iterations, doubling) and returns 7 WITHOUT having enqueued anything --
 *     re-issue it; dbm_timeout_info says how many queued updates were dropped.  Entry points that take HOST pointers and
 *     therefore end with a stream synchronisation (dbm_gen_forward / dbm_gen_backward -- the calls that launch persistent kernels --
 *     dbm_disc_forward and the loss calls, without DBM_DEVICE_PTRS) observe the condition after that synchronisation as well: their
 *     results are void, status 7.  FORWARD and loss calls are simply re-issued.  dbm_gen_backward / dbm_disc_backward are NOT: gradients
 *     accumulate, so after status 7 from a backward call: dbm_model_cleargrads, then repeat forward AND backward.
 *     dbm_adam_update is the other exception: whenever an event has been handled (by any call) since the model's gradient arena
 *     was last cleared, the arena may hold the sums of a void pass -- it returns status 9, applies nothing, and the caller clears
 *     the gradients and repeats forward + backward before updating (the step entry points clear them themselves).  Status 8:
 *     the same in a data-parallel run, where a local retry cannot keep the replicas identical -- fatal, abort the job.  Status 10
 *     (dbm_grid_tension_surface only): the solve did not converge within max_iter; the output holds the last iterate.  Status 11
 *     (dbm_tiff_decode only): a block's LZW or deflate stream is malformed.  Status 12 (dbm_tiff_encode, dbm_chunk_encode, dbm_png_encode): a block's LZW or deflate stream
 *     did not fit its slot (the guard of the device encoders; it cannot occur with the slot the calls allocate);
 *   - tensors are NCHW float32, C-contiguous; weights OIHW, exactly the arrays stored by
 *     chainer.serializers.save_npz (key layout: SURVEY.md Appendix B);
 *   - pointers are HOST pointers unless flags contains DBM_DEVICE_PTRS, in which case they are
 *     device pointers on the context's GPU and the call only enqueues work on the context's
 *     stream (no synchronisation);
 *   - a dbm_ctx is bound to one GPU and one HIP stream and is not thread-safe; data parallelism
 *     is one process (one ctx) per GPU.
 */
#ifndef DBM_H
#define DBM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dbm_ctx dbm_ctx;
typedef struct dbm_model dbm_model;

enum {
  DBM_DEVICE_PTRS = 1, /* array arguments are device pointers; call is asynchronous on the ctx stream */
  DBM_KEEP_GRAPH = 2,  /* retain activations for a following backward (Chainer: enable_backprop=True) */
  DBM_BF16 = 8,        /* dbm_gen_forward without DBM_KEEP_GRAPH: the convolutions multiply in bf16 (operands rounded to
                          nearest-even, fp32 accumulation, fp32 storage): the area-inference mode of BASELINE config 5 */
  DBM_BN_TRAIN = 4,    /* discriminator BatchNorm uses batch statistics and updates running stats
                          (chainer.config.train=True, srgan_train.py:1125) */
  DBM_ONE_GEN_FORWARD = 16 /* dbm_train_iteration (opt-in, not the reference's call sequence): the generator runs ONCE per
                          minibatch -- the G-step's retained forward also supplies the D-step's fakes (same weights, same
                          inputs: srgan_train.py:1131-1137 and :1222-1227 compute the same images); bit for bit the two step calls
                          with their share flag, and the default iteration up to fp32 rounding (the unretained pass sums
                          conv_layer5 of the trunk in another order) */
};
enum { DBM_KIND_PARAM = 0, DBM_KIND_PERSISTENT = 1 };
/* dbm_points_*: threads per workgroup of the point passes, and the largest block population of each size class of the block
 * medians' selection (points.hip: 8 lanes, 32 lanes, one wavefront, one workgroup sorting in LDS; anything larger is selected
 * out of global memory).  Constants of the sources, listed here so that tests can build clouds on both sides of every boundary. */
enum {
  DBM_POINTS_THREADS = 256,
  DBM_BLOCKMEDIAN_SUB8 = 8,
  DBM_BLOCKMEDIAN_SUB32 = 32,
  DBM_BLOCKMEDIAN_WAVE = 64,
  DBM_BLOCKMEDIAN_LDS = 2048,
  DBM_BLOCKMEDIAN_CLASSES = 5
};
/* dbm_grid_polygon_mask: the side of a node tile (one 256-thread workgroup classifies TILE x TILE nodes) and the number of edges a
 * workgroup stages into LDS at a time (polygon.hip).  Listed here so that tests can put grids and edge counts on both sides of them. */
enum {
  DBM_POLY_TILE = 16,
  DBM_POLY_CHUNK = 256
};
/* dbm_image_overlay: the two kinds of primitives, the side of a pixel tile (one 256-thread workgroup paints TILE x TILE pixels) and the
 * number of primitives a workgroup stages into LDS at a time (overlay.hip).  Listed here so that tests can put images and primitive
 * counts on both sides of them. */
enum { DBM_OVERLAY_SEGMENTS = 0, DBM_OVERLAY_DISCS = 1 };
enum {
  DBM_OVERLAY_TILE = 16,
  DBM_OVERLAY_CHUNK = 256
};
/* dbm_text_*: bytes of text a workgroup stages and parses the lines of, its threads (text.hip: a thread owns the lines that start in
 * its TILE_BYTES / THREADS bytes), the separator value that stands for runs of spaces and tabs (`\s+`), and the limits of the reader
 * description.  Listed here so that tests can put newlines, numbers and long lines on both sides of every tile edge. */
enum {
  DBM_TEXT_TILE_BYTES = 16384,
  DBM_TEXT_THREADS = 256,
  DBM_TEXT_SEP_WHITESPACE = 256,
  DBM_TEXT_MAX_FIELDS = 64,
  DBM_TEXT_MAX_NA = 8,
  DBM_TEXT_MAX_NA_BYTES = 16,
  DBM_TEXT_MAX_COLUMNS = 8
};
/* dbm_track_error_*: the most probabilities of one quantile call, the most bins of one histogram, the bytes of device workspace either
 * call fits in, and the threads and the most workgroups of their passes over the points (track_dist.hip).  Listed here so that tests
 * can put n on both sides of a workgroup's share and of one grid-stride round. */
enum {
  DBM_TRACK_MAX_QUANTILES = 16,
  DBM_TRACK_MAX_BINS = 4096,
  DBM_TRACK_DIST_WORKSPACE = 69632,
  DBM_TRACK_DIST_THREADS = 256,
  DBM_TRACK_DIST_BLOCKS = 1024
};

/* ---- context ---- */
int dbm_init(int hip_device, dbm_ctx** out);      /* replaces model.to_gpu(): srgan_train.py:1038-1040, deepbedmap.py:659 */
int dbm_shutdown(dbm_ctx* ctx);
const char* dbm_last_error(dbm_ctx* ctx);         /* ctx may be NULL (error of a failed dbm_init) */
int dbm_set_stream(dbm_ctx* ctx, void* hip_stream); /* run on a caller-owned hipStream_t (NULL = the ctx's own) */
int dbm_synchronize(dbm_ctx* ctx);
/* chainer.global_config.cudnn_deterministic (srgan_train.py:69, deepbedmap.py:689).  on = 1: every gradient is folded in a
 * fixed order (no fp32 atomics over a K split: partial sums + an ordered fold kernel, sorted sampling lists, a separate
 * offset-gradient kernel), so a training run is bitwise reproducible; costs a few per cent.  Default 1, the reference's
 * setting.  Process-wide. */
int dbm_set_deterministic(dbm_ctx* ctx, int on);
/* sync_batch_stats (data-parallel training that must equal ONE process at the global batch): with world > 1 the
 * discriminator's training-mode BatchNorm layers (srgan_train.py:636-644, 663-689) use the statistics of the global batch in
 * forward and backward, and calculate_discriminator_loss (srgan_train.py:995-1004) the global-batch means of the logits.
 * The library computes per-rank sums into a small device buffer and calls allreduce_sum(user, dev, n), which must enqueue
 * an in-place SUM all-reduce of n floats on the context's stream (RCCL / torch.distributed on the shared stream).
 * With a native communicator of the same world (dbm_comm_init) the hook may be NULL: the sums go through RCCL.
 * world = 1 restores per-rank statistics, the default. */
int dbm_set_sync_batch_stats(dbm_ctx* ctx, int world, void (*allreduce_sum)(void* user, float* dev, int n), void* user);
/* ---- gradient exchange of a data-parallel run (one process / one dbm_ctx per GPU) ----
 * The reference trains on ONE GPU (srgan_train.py:58-61, 1039-1040: `model.to_gpu()` of a single device); these entry
 * points are what a multi-GPU `trainer` (srgan_train.py:1267-1329) calls between `backward()` and `optimizer.update()`
 * (:1163-1164, :1256-1257).  Native path: RCCL over xGMI, opened at run time (librccl.so.1), no torch involved.
 * dbm_comm_unique_id: rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other ranks by
 * any host channel; dbm_comm_init: every rank joins (collective call; world = 1 is allowed and makes everything below a
 * no-op).  With a communicator on the context, dbm_discriminator_step / dbm_generator_step sum their gradient arenas
 * over ranks THEMSELVES, bucket by bucket underneath the backward passes (D: conv_layer6..9 = 89 % of the bytes as soon
 * as their weight gradients are enqueued, the rest at the end; G: tail, trunk groups, input block), on a library
 * stream; the caller then runs dbm_adam_update(m, 1.0 / world).  Bit 4 (16) of `train` leaves the exchange to the caller.
 * dbm_comm_set_hook replaces RCCL by a callback (tests: several ranks on one GPU, where RCCL refuses to run): it must
 * enqueue an in-place SUM all-reduce of n floats ordered after the work already enqueued on hip_stream and before
 * work enqueued there later (a blocking implementation may synchronise that stream and reduce on the host). */
int dbm_comm_unique_id(void* out128);
int dbm_comm_init(dbm_ctx* ctx, int rank, int world, const void* id128);
int dbm_comm_set_hook(dbm_ctx* ctx, int rank, int world,
                      void (*allreduce_sum)(void* user, float* dev, size_t n, void* hip_stream), void* user);
int dbm_comm_destroy(dbm_ctx* ctx);
/* in-place broadcast / sum all-reduce of device floats on the context's stream (parameter broadcast at start-up; metrics) */
int dbm_comm_broadcast(dbm_ctx* ctx, float* dev, size_t nfloats, int root);
int dbm_comm_allreduce(dbm_ctx* ctx, float* dev, size_t nfloats);
/* bytes / collective calls issued so far on this context's communicator (reset != 0 clears the counters) */
int dbm_comm_stats(dbm_ctx* ctx, int* world, size_t* bytes, size_t* calls, int reset);

/* measurement aid (bench.py roofline leg): while enabled, every launch of the two MFMA kernel families is bracketed
 * by hipEvents on the launch stream.  out = [ms, algorithmic FLOP, launches] for igemm_conv_kernel (forward + data
 * gradient), then the same three for wgrad_kernel. */
int dbm_profile_begin(dbm_ctx* ctx);
int dbm_profile_end(dbm_ctx* ctx, double out[8]);
/* the same for nfam <= 5 kernel families, three values each: igemm_conv_kernel, the weight-gradient kernels,
 * trunk_fused_kernel (RRDB trunk forward, srgan_train.py:546), trunk_fused_bwd_kernel (its data-gradient chain),
 * trunk_fused_kernel in the form with a helper workgroup per image (passes that keep nothing; nfam <= 4: counted with the
 * third family) */
int dbm_profile_end_ex(dbm_ctx* ctx, double* out, int nfam);
/* the same brackets with the device synchronised before and after every bracketed launch: STANDALONE launch durations
 * (inside a training step up to four streams share the chip and every bracket also contains the neighbours' work).
 * Ended by dbm_profile_end_ex. */
int dbm_profile_begin_serial(dbm_ctx* ctx);
/* ends either kind of bracketing and returns EVERY bracket as a text line "family flops bytes ms wgs tag\n": family as in
 * dbm_profile_end_ex (0..4), the launch's algorithmic FLOP and algorithmic BYTES (operands read once + results written once),
 * its duration, its workgroup count (what joins a bracket to a rocprofv3 dispatch row) and a label of its shape (layer geometry) -- bench.py's per-shape roofline table, and the denominator of the
 * traffic ratio in profiles/<round>/traffic_pmc.json.  *len = the text's length; if it does not fit into cap (with its NUL)
 * nothing is copied and the text is kept for a second call with a larger buffer. */
int dbm_profile_end_records(dbm_ctx* ctx, char* buf, size_t cap, size_t* len);
/* testing aid: raises the condition a persistent trunk kernel raises when it gives up waiting for a neighbouring
 * workgroup.  From then on the optimizer launches and BatchNorm's running-average writes are no-ops; the next STEP entry
 * point (or dbm_check_timeout) returns status 7 without enqueuing anything. */
int dbm_debug_inject_timeout(dbm_ctx* ctx);
/* the same raised by a kernel ENQUEUED on the context's stream (no host synchronisation): the condition comes up in stream
 * order, as a persistent kernel's would, with whatever the host has queued behind it running under the raised flag */
int dbm_debug_inject_timeout_async(dbm_ctx* ctx);
/* Observes a pending persistent-kernel timeout like the step entry points do (status 7 / 8, see the conventions above); 0
 * when there is none.  For the end of an epoch: the last iterations of a run have no following step call that would
 * notice.  (srgan_train.py has no counterpart: Chainer's kernels cannot time out.) */
int dbm_check_timeout(dbm_ctx* ctx);
/* What the last handled timeout cost: number of events so far, optimizer updates of the discriminator / generator that
 * were no-ops (= minibatches whose update was dropped), and whether the persistent trunk kernels are currently paused.
 * Any pointer may be NULL. */
int dbm_timeout_info(dbm_ctx* ctx, long* events, int* d_updates_skipped, int* g_updates_skipped, int* persistent_off);
/* measurement aid: HIP-event stopwatch on the context's stream.  op 0 = record the start event, 1 = record the stop
 * event (both asynchronous), 2 = wait for the stop event and write the elapsed milliseconds to *ms. */
int dbm_timer(dbm_ctx* ctx, int op, double* ms);
/* measurement aid: while enabled, the step entry points record one hipEvent per phase boundary on the main stream;
 * enable = 0 stops, synchronises and writes "name milliseconds-since-the-first-mark" lines into out (cap bytes). */
int dbm_phase_marks(dbm_ctx* ctx, int enable, char* out, int cap);
int dbm_malloc(dbm_ctx* ctx, size_t bytes, void** dptr);
int dbm_free(dbm_ctx* ctx, void* dptr);
int dbm_memcpy_h2d(dbm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int dbm_memcpy_d2h(dbm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* device-resident area inference (deepbedmap.py:706-737: the per-tile `xp.asarray(...)` crops and the paste into Y_hat,
 * without leaving HBM): pitched device-to-device copy of `height` rows of `width_bytes`, and a float fill (NaN canvas).
 * Asynchronous on the context's stream. */
int dbm_memcpy2d_d2d(dbm_ctx* ctx, void* dst_dev, size_t dst_pitch, const void* src_dev, size_t src_pitch,
                     size_t width_bytes, size_t height);
int dbm_fill_f32(dbm_ctx* ctx, float* dst_dev, size_t n, float value);
/* `np.clip(a=W_tile, a_min=0.0, a_max=None)` (deepbedmap.py:663-665: ice surface elevation, velocity and accumulation are
 * clipped to >= 0 before the sweep) on a grid that already lives in HBM: in place, NaN stays NaN.  Asynchronous. */
int dbm_clip_min_f32(dbm_ctx* ctx, float* dst_dev, size_t n, float lo);
/* chainer.dataset.concat_examples over a dataset that lives on the device (srgan_train.py:107-121 `to_gpu`, 1286-1288):
 * dst row i = src row idx[i], rows of row_bytes (a multiple of 4) bytes; idx is a HOST array of n ints.  Asynchronous. */
int dbm_gather_rows(dbm_ctx* ctx, void* dst_dev, const void* src_dev, const int* idx_host, int n, size_t row_bytes);

/* ---- models ---- */
/* GeneratorModel.__init__(num_residual_blocks=12, residual_scaling=0.1, out_channels=1): srgan_train.py:450-523.
 * Parameters are created zero; the caller uploads them (HeNormal init or load_npz) with dbm_model_set_tensor.
 * out_channels in [1, 16]; more than one channel is forward-only (y is (N, out_channels, 4(H-2), 4(W-2))): the reference's
 * own training step fails with it (F.mean_absolute_error against the one-channel x_topo, srgan_train.py:882-883). */
int dbm_gen_create(dbm_ctx* ctx, int num_residual_blocks, float residual_scaling, int out_channels, dbm_model** out);
/* DiscriminatorModel.__init__(): srgan_train.py:611-647 */
int dbm_disc_create(dbm_ctx* ctx, dbm_model** out);
int dbm_model_destroy(dbm_model* m);
/* Link.namedparams()/serialize(): tensors in chainer.serializers.save_npz key order -- srgan_train.py:1355-1361, deepbedmap.py:408 */
int dbm_model_num_tensors(dbm_model* m, int* n);
int dbm_model_tensor_info(dbm_model* m, int i, const char** npz_key, int* ndim, int64_t shape[4], int* kind);
int dbm_model_set_tensor(dbm_model* m, const char* npz_key, const float* host, size_t nfloats);
int dbm_model_get_tensor(dbm_model* m, const char* npz_key, float* host, size_t nfloats);
int dbm_model_get_grad(dbm_model* m, const char* npz_key, float* host, size_t nfloats);
/* Link.count_params(): srgan_train.py:446, 607 */
int dbm_model_count_params(dbm_model* m, int64_t* n);
/* Link.cleargrads(): srgan_train.py:1162, 1255 */
int dbm_model_cleargrads(dbm_model* m);
/* flat fp32 arenas (device pointers) holding every parameter / gradient contiguously in tensor order:
 * what a data-parallel host all-reduces (RCCL) between backward and update */
int dbm_model_param_arena(dbm_model* m, void** dptr, size_t* nfloats);
int dbm_model_grad_arena(dbm_model* m, void** dptr, size_t* nfloats);
/* tell the library the parameter arena was written from outside (e.g. an RCCL broadcast) so that its packed
 * MFMA weight images are rebuilt before the next forward */
int dbm_model_params_changed(dbm_model* m);

/* ---- forward / backward ---- */
/* GeneratorModel.forward(x, w1, w2, w3): srgan_train.py:525-576.  x (N,1,H,W), w1 (N,1,10H,10W), w2 (N,2,2H,2W),
 * w3 (N,1,H,W) -> y (N,1,4(H-2),4(W-2)).  flags: DBM_DEVICE_PTRS, DBM_KEEP_GRAPH, DBM_BF16.
 * Plane limits (input tile H x W, output H4 x W4 = 4(H-2) x 4(W-2)); every other size runs if it fits in memory:
 *   - refused (DBM_CHECK) when N * H4 * W4 >= 2^31: "fused deformable convolution: more than 2^31 positions" / "igemm: more than
 *     2^31 output positions" (the launchers index positions in 32 bits);
 *   - DBM_BF16 only: refused up front when (H-2) * (W-2) > 5592405 ("dbm_gen_forward: DBM_BF16 needs ..."): the bf16 trunk's
 *     conv_cl16 launches address a 192-channel bf16 concat per image at 32-bit byte offsets (launch_conv_cl16 itself refuses
 *     "cl16 conv: one image plane must stay below 2 GiB per operand"); the fp32 forward serves those planes;
 *   - not limits: the deformable layers' LDS-window kernels serve H4 <= 32765, W4 <= 65533, H4 * W4 < 2^24 only, the launchers take
 *     the gathering kernels (64-bit offsets, the same bits) past them; conv_tile's LDS form hands planes whose 32-bit epilogue
 *     offsets would overflow to the implicit GEMM (64-bit offsets).
 * tests/test_gpu_large_planes.py holds a case on each side of each limit. */
int dbm_gen_forward(dbm_model* g, int N, int H, int W, const float* x, const float* w1, const float* w2,
                    const float* w3, float* y, int flags);
/* g_loss.backward() through the generator: srgan_train.py:1256.  gy (N,1,4(H-2),4(W-2)) = d loss / d y of the last
 * DBM_KEEP_GRAPH forward; accumulates into the gradient arena. */
int dbm_gen_backward(dbm_model* g, const float* gy, int flags);
/* DiscriminatorModel.forward(x): srgan_train.py:649-699.  img (N,1,36,36) -> logits (N,1).
 * slot (0/1) selects which retained graph a DBM_KEEP_GRAPH call fills (the D-step runs real and fake batches). */
int dbm_disc_forward(dbm_model* d, int N, int H, int W, const float* img, float* logits, int flags, int slot);
int dbm_disc_backward(dbm_model* d, int slot, const float* glogits, int flags);

/* ---- losses / metrics ---- */
/* calculate_discriminator_loss: srgan_train.py:960-1009 (+ F.binary_accuracy :1156-1158).
 * out[0] = loss, out[1] = accuracy; g_real/g_fake (N) may be NULL. */
int dbm_discriminator_loss(dbm_ctx* ctx, const float* real_logits, const float* fake_logits, int N,
                           int real_minus_fake_target, int fake_minus_real_target, float* out2, float* g_real,
                           float* g_fake, int flags);
/* the same with per-sample int32 target arrays (N each; 0, 1 or -1 = ignored), what the reference's signature accepts
 * (srgan_train.py:960-1004: `real_minus_fake_target`, `fake_minus_real_target` are arrays handed to
 * F.sigmoid_cross_entropy, each call normalised by its count of targets != -1) */
int dbm_discriminator_loss_t(dbm_ctx* ctx, const float* real_logits, const float* fake_logits, int N,
                             const int* real_minus_fake_target, const int* fake_minus_real_target, float* out2, float* g_real,
                             float* g_fake, int flags);
/* calculate_generator_loss: srgan_train.py:841-902, psnr :906-928, ssim_loss_func :932-956.
 * y_pred,y_true (N,1,H,W); x (N,1,H/4+2,W/4+2) is the full BEDMAP2 tile (x_topo = x[:,:,1:-1,1:-1], :1248);
 * fake_logits (N) from the discriminator in eval mode, real_logits (N) or NULL for the reference's ones(N) (:1233);
 * the adversarial term is calculate_discriminator_loss(real, fake, real_minus_fake_target, fake_minus_real_target)
 * (:874-879; the G-step passes targets 0 and 1, :1236-1237).  weights[4] = content, adversarial, topographic,
 * structural.  out[0] = g_loss, out[1] = psnr, out[2] = ssim; gy (N,1,H,W) may be NULL (the adversarial term is
 * detached from y_pred, :1228-1229).  ssim_window: 0 gaussian(1.5), 1 uniform. */
int dbm_generator_loss(dbm_ctx* ctx, const float* y_pred, const float* y_true, const float* x,
                       const float* real_logits, const float* fake_logits, int N, int H, int W,
                       const float weights[4], int real_minus_fake_target, int fake_minus_real_target,
                       int ssim_window, float* out3, float* gy, int flags);
/* the same with per-sample int32 target arrays for the adversarial term (see dbm_discriminator_loss_t) */
int dbm_generator_loss_t(dbm_ctx* ctx, const float* y_pred, const float* y_true, const float* x,
                         const float* real_logits, const float* fake_logits, int N, int H, int W,
                         const float weights[4], const int* real_minus_fake_target, const int* fake_minus_real_target,
                         int ssim_window, float* out3, float* gy, int flags);

/* psnr(y_pred, y_true, data_range=2**32): srgan_train.py:906-928 over n elements; out[0] = 20*log10(range/sqrt(mse)) */
int dbm_psnr(dbm_ctx* ctx, const float* y_pred, const float* y_true, size_t n, double data_range, float* out,
             int flags);
/* ssim_loss_func(y_pred, y_true, window_size=9, stride=1): srgan_train.py:932-956; (N,1,H,W), H,W >= 9 */
int dbm_ssim(dbm_ctx* ctx, const float* y_pred, const float* y_true, int N, int H, int W, int ssim_window,
             float* out, int flags);
/* ssim_loss_func with any window_size (1..64, gaussian(1.5) centred at window_size / 2 or uniform) and stride >= 1:
 * the metric for other windows than the loss's 9 / 1 (valid windows only; N counts images x channels) */
int dbm_ssim_ex(dbm_ctx* ctx, const float* y_pred, const float* y_true, int N, int H, int W, int window_size, int stride,
                int ssim_window, float* out, int flags);

/* ---- evaluation: `gmt.grdtrack(points, grid)` and the along-track error (srgan_train.py:1458-1464, the test-area RMSE that
 * get_deepbedmap_test_result returns; deepbedmap.py:530-574, the product grids' elevation error) ----
 * The float32 grid (H, W) -- ALWAYS a device pointer, row r, column c at (x0 + c dx, y0 + r dy), geom = {x0, y0, dx, dy,
 * registration (0 gridline: domain [0, W-1] x [0, H-1] in node units; 1 pixel: [-1/2, W-1/2] x [-1/2, H-1/2])} on the host --
 * is evaluated in float64 at the n points (C-contiguous float64 (n, ncol), ncol 2: x, y; 3: x, y, z) with GMT's interpolant
 * (`grdtrack -n`): interp 0 nearest, 1 bilinear, 2 bicubic (Keys cubic convolution, a = -1/2).  Outside the domain, or at NaN
 * coordinates: NaN.  Ghost nodes beyond the edges: linear extrapolation (columns first, then rows).  NaN nodes: the valid nodes'
 * weighted sum over their weight sum if that sum + 1e-9 >= threshold (GMT's +t, default 0.5), else NaN.
 * z_out (n doubles, may be NULL) receives z_interpolated; with ncol 3 and stats != NULL the finite errors z_interpolated - z
 * are reduced to stats = {count, mean, std (ddof 1), min, max, rmse} (count 0: the rest NaN; std NaN below 2), bit for bit the
 * same from call to call (no float atomics; the launch depends on n only).  flags: DBM_DEVICE_PTRS = points, z_out and stats
 * are device pointers (asynchronous); otherwise host pointers and the call synchronises.  Refused (status 1, nothing
 * launched): interp outside 0..2, H or W < 1, H or W < 2 for bilinear / bicubic, threshold outside (0, 1], ncol not 2 or 3,
 * dx or dy zero or not finite. */
int dbm_grid_track(dbm_ctx* ctx, const float* grid_dev, long H, long W, const double geom[5], const double* points, size_t n,
                   int ncol, int interp, double threshold, double* z_out, double* stats, int flags);

/* ---- the rest of the error table and the error histogram (deepbedmap.py:550-563, the 25 %, 50 % and 75 % rows of `df.describe()` of
 * error = z_interpolated - z; deepbedmap.py:575-608, `df.hist(column="error", bins=25)`) ----
 * Both calls take the points table -- C-contiguous float64 (n, 3) x, y, z -- and the z_interpolated column (n doubles) that
 * dbm_grid_track wrote for it, and work on e_i = z_interpolated_i - z_i, formed on the fly in float64.  An error takes part iff it is
 * finite (the set dbm_grid_track reduces; m of them) and -0.0 counts as +0.0.  flags: DBM_DEVICE_PTRS = points, z_interpolated and the
 * result are device pointers (asynchronous); otherwise host pointers, staged, and the call synchronises.  probabilities and edges are
 * ALWAYS host pointers (read before the call returns).  workspace_dev: DBM_TRACK_DIST_WORKSPACE bytes of device memory, 256-byte
 * aligned, the call's own until its work on the stream is done; NULL: the call allocates and frees it, which synchronises.  Only
 * integer atomics carry counts between lanes and workgroups (no float atomics): every result is exact, the same bytes from call to
 * call and under any permutation of the points.
 *
 * dbm_track_error_quantiles: quantiles_out[k] = `np.quantile(e, probabilities[k], method="linear")` of the m finite errors (what
 * `Series.describe()` and `Series.quantile` compute), count in 1..DBM_TRACK_MAX_QUANTILES probabilities in any order, duplicates
 * allowed.  Exact order statistics by a device-wide radix select -- no sort: errors map to order-preserving 64-bit keys, eight digit
 * passes read the points once each (however many probabilities are asked) and count, per wanted rank, the next digit of the keys that
 * share the rank's prefix; one workgroup narrows the prefixes between the passes; no host round trip.  Then h = (m - 1) q, j = floor(h),
 * g = h - j; a, b = the order statistics j and j + 1 (both the maximum if h >= m - 1); d = b - a; the result is a + d g, or
 * b - d (1 - g) where g >= 0.5, every product and sum rounded on its own (no fused multiply-add).  m = 0: NaN.
 *
 * dbm_track_error_histogram: counts_out (bins int64) = `np.histogram(e, bins=bins, range=(edges[0], edges[bins]))[0]` for the
 * bins + 1 edges the caller computed (`np.linspace(first, last, bins + 1)`), by NumPy's uniform-bin rule: keep first <= e <= last;
 * i = (long)(((e - first) / (last - first)) * bins), an IEEE division; i == bins: i - 1; e < edges[i]: i - 1; e >= edges[i + 1] and
 * i != bins - 1: i + 1 (the last bin includes its right edge).
 *
 * Refused (status 1, nothing launched or written): NULL pointers with n > 0, NULL probabilities / edges / result, n >= 2^40, count
 * outside 1..DBM_TRACK_MAX_QUANTILES, a probability that is NaN or outside [0, 1], bins outside 1..DBM_TRACK_MAX_BINS, edges that are
 * not finite, that decrease, or with edges[0] >= edges[bins]. */
int dbm_track_error_quantiles(dbm_ctx* ctx, const double* points, const double* z_interpolated, size_t n, const double* probabilities,
                              int count, double* quantiles_out, void* workspace_dev, int flags);
int dbm_track_error_histogram(dbm_ctx* ctx, const double* points, const double* z_interpolated, size_t n, const double* edges, int bins,
                              int64_t* counts_out, void* workspace_dev, int flags);

/* ---- tiling: `selective_tile` (data_prep.py:622-741: every raster cut and bilinearly geo-registered to a list of windows; the
 * training set data_prep.py:757-771, 880-911 and the inputs of an area deepbedmap.py:132-213 are built from it) ----
 * The float32 raster (H, W) -- ALWAYS a device pointer, node (r, c) at (x0 + c dx, y0 + r dy), geom = {x0, y0, dx, dy}, either sign --
 * is cut into n tiles of (out_h, out_w): out_dev[k * window_stride + r * out_w + c] (device, window_stride in floats: with
 * window_stride = 2 * out_h * out_w two calls fill the two channels of an (n, 2, h, w) array).  windows_host is a HOST array of
 * 32 bytes per window, staged like dbm_gather_rows' indices; the call is asynchronous on the context's stream.
 * mode 1 (interpolate=True): windows = (left, bottom, right, top) doubles, already padded.  Tile row r, column c is the raster at
 * y = np.linspace(top - res/2, bottom + res/2, out_h)[r], x = np.linspace(left + res/2, right - res/2, out_w)[c] (float64, NumPy's
 * bits: multiply, then add, the end point exact), interpolated as scipy.interpolate.interpn(method="linear") does it: axes sorted
 * ascending, node coordinates x0 + j dx, cell i with g[i] <= c < g[i+1] (last node: i = n - 2, t = 1), NaN outside [g[0], g[n-1]]
 * or at a NaN coordinate, the float64 sum of z * (wy * wx) over all four nodes with zero weights included (a NaN node makes its
 * whole closed cell NaN), no fused multiply-add.
 * mode 0 (interpolate=False, `sel(method="nearest", tolerance=0)`): windows = (row0, col0, row step, column step) int64, steps +-1,
 * a pure copy; the caller has checked that the tile's coordinates ARE node coordinates.
 * Masking (data_prep.py:699-730, numpy.ma.masked_values applied after the interpolation): with nodata != NULL and *nodata not NaN a
 * value v is masked iff |v - nodata| <= 1e-8 + 1e-5 |nodata| (v in float64, before rounding); NaN values are not masked unless
 * fill_nan (an extension); masked values become *gapfiller if gapfiller != NULL; counts_dev (n ints, device, may be NULL) receives
 * the number of masked values per window.  Values are rounded to float32 once, at the end.
 * Refused (status 1, nothing launched): mode outside 0..1, n < 0, out_h or out_w < 1, H or W < 2 for mode 1, dx or dy zero or not
 * finite, a resolution that is not positive (mode 1), window_stride < out_h * out_w, a NULL raster, window list or output with
 * n > 0, a nodata that is infinite, a mode 0 window that leaves the raster.  n = 0 succeeds and does nothing. */
int dbm_grid_tile(dbm_ctx* ctx, const float* grid_dev, long H, long W, const double geom[4], const void* windows_host, long n, int mode,
                  double resolution, int out_h, int out_w, const double* nodata, const float* gapfiller, int fill_nan, float* out_dev,
                  size_t window_stride, int* counts_dev);
/* `get_window_bounds` (data_prep.py:501-572: `view_as_windows(mask, (height, width), step)` and `~any`): flags_dev[uly * nx + ulx]
 * (device bytes, ny = (H - size) / step + 1 rows of nx = (W - size) / step + 1) = 1 iff no node of rows [uly step, uly step + size)
 * x columns [ulx step, ulx step + size) is NaN.  Rows are counted from the NORTH edge (flip_rows != 0: raster row 0 is the south
 * edge), columns from the west (flip_cols != 0: raster column 0 is the east edge).  Asynchronous.  `argwhere` and the bounds stay
 * with the caller.  Refused (status 1): size odd, < 2 or > 8192, step < 1, H or W < size, NULL pointers. */
int dbm_grid_filled_windows(dbm_ctx* ctx, const float* grid_dev, long H, long W, int size, int step, int flip_rows, int flip_cols,
                            unsigned char* flags_dev);
/* Gap filling of a fine raster from a coarse one (data_prep.py:838-877: REMA at 100 m patched from the 200 m mosaic).  fine_dev
 * (H, W) float32, north-up, is the raster whose pixel edges are bounds = {minx, miny, maxx, maxy} at `resolution`.  out_dev[r, c] =
 * fine_dev[r, c] bit for bit unless that value is NaN or (fine_nodata != NULL, *fine_nodata not NaN) equals (float)*fine_nodata; at
 * such a node it is what dbm_grid_tile(coarse_dev, mode 1, windows = {bounds}, resolution, out_h = H, out_w = W, no gap filler)
 * writes at [r, c]: the package's bilinear rule above (the same code), NaN outside the coarse raster, a coarse nodata value
 * interpolated like any other (mask it afterwards if need be).  This is NOT GDAL's mask-renormalised resampler.
 * out_dev may be fine_dev (in place: only the gap nodes are written).  Asynchronous on the context's stream.  Refused (status 1,
 * nothing launched): NULL pointers, H or W outside 1..2^31 - 1, cH or cW < 2, coarse_geom = {x0, y0, dx, dy} not finite or with a
 * zero spacing, bounds not finite, a resolution that is not positive, an infinite nodata, out_dev == coarse_dev. */
int dbm_grid_fill_gaps(dbm_ctx* ctx, const float* fine_dev, long H, long W, const double bounds[4], double resolution, const double* fine_nodata,
                       const float* coarse_dev, long cH, long cW, const double coarse_geom[4], float* out_dev);

/* ---- comparison grids: the bicubic BEDMAP2 baseline and the synthetic grid at 250 m (deepbedmap.py:323-331, 348-356:
 * `skimage.transform.rescale(image.astype(np.int32), scale, order, mode="reflect", anti_aliasing=True, preserve_range=True)`; again at
 * paper_figures.py:893-917), whose track error is set against DeepBedMap's (deepbedmap.py:550-574, 622-626) ----
 * The float32 grid (H, W) -> out_dev (out_h, out_w), both DEVICE pointers, asynchronous on the context's stream, by the scipy.ndimage
 * chain that current scikit-image releases run for `rescale` (the caller computes out = round(scale * in)): with input_cast the values
 * are truncated toward zero first (`.astype(np.int32)`); with anti_aliasing each axis with factor = in / out > 1 is filtered by
 * gaussian_filter(sigma = (factor - 1) / 2, mode="mirror", truncate 4: radius int(4 sigma + 0.5)), axis 0 first; order 3 prefilters both
 * axes (pole sqrt(3) - 2, gain 6, mirror start values); output node o samples the input coordinate (o + 0.5) in / out - 0.5 (zoom with
 * grid_mode=True, mode="mirror") with linear (order 1) or cubic B-spline (order 3) weights; with clip the result is clamped to [min, max]
 * of the (cast) input.  Float64 throughout, rounded to float32 once; the same bits from call to call.  NaN or infinite nodes are outside
 * the contract (the recursive filter spreads them over rows and columns, as scipy's does).  The pinned scikit-image 0.15 of the reference
 * interpolates differently.  Refused (status 1, nothing launched): order not 1 or 3, H or W < 2, out_h or out_w < 1, NULL
 * pointers, out_dev == in_dev. */
int dbm_grid_rescale(dbm_ctx* ctx, const float* in_dev, long H, long W, long out_h, long out_w, int order, int anti_aliasing, int clip,
                     int input_cast, float* out_dev);
/* `standard_deviation_2d(grid, window_length)` (paper_figures.py:847-867, used at :928-931 and sampled along a transect at :989-998):
 * out_dev[r, c] (device) = the population standard deviation (ddof 0) of the non-NaN nodes of rows r - h .. r + h, columns c - h .. c + h
 * (h = window / 2) that lie inside the grid, NaN where there is none; float64 sums of values shifted by one valid node of the window
 * (a constant window gives exactly 0), rounded to float32 once.  Asynchronous.  Refused (status 1): window even or outside 1..63, H or
 * W < 1, NULL pointers, out_dev == in_dev. */
int dbm_grid_rolling_std(dbm_ctx* ctx, const float* in_dev, long H, long W, int window, float* out_dev);

/* ---- gridding: survey point clouds -> the `points` table and the 250 m ground-truth raster (data_prep.py:322-334 the
 * `filters.reprojection` step of ascii_to_xyz; :353-378 get_region; :406-407 the `gmt.blockmedian` preprocessing of xyz_to_grid) ----
 * Point tables are C-contiguous float64 (n, ncol), as dbm_grid_track takes them; all arithmetic is float64.  flags: DBM_DEVICE_PTRS =
 * the table arguments are device pointers; otherwise host pointers, staged, and the call synchronises.  NOT built:
 * `gmt info -Is<inc>` (the surface-friendly widening).  The CSV reading of ascii_to_xyz: dbm_text_*, below.  The second half of xyz_to_grid -- a tension
 * surface through the block medians, the distance mask and `grdsample -T` -- is the next group of entry points (it is this project's own,
 * fully defined surface, NOT a reproduction of GMT `surface`: DESIGN.md 6f).
 *
 * dbm_points_polar_stereographic (data_prep.py:322-334, what pyproj's EPSG:4326 -> EPSG:3031 transformer computes): EPSG method 9829
 * (Polar Stereographic, variant B), south-pole case, Guidance Note 7-2.  Columns 0 and 1 -- longitude, latitude in degrees -- become
 * easting, northing in metres; columns 2.. are copied unchanged.  proj = {a, 1/f, latitude of true scale (degrees, < 0), longitude of
 * origin (degrees), false easting, false northing}; EPSG:3031 is {6378137, 298.257223563, -71, 0, 0, 0}.  With e^2 = 2f - f^2,
 * C = sqrt((1+e)^(1+e) (1-e)^(1-e)): t = tan(pi/4 + phi/2) / ((1 + e sin phi) / (1 - e sin phi))^(e/2), m_F = cos phi_F /
 * sqrt(1 - e^2 sin^2 phi_F), k0 = m_F C / (2 t_F), rho = 2 a k0 t / C, E = FE + rho sin(lambda - lambda0), N = FN + rho cos(lambda -
 * lambda0); the constants are computed once on the host.  A non-finite longitude or latitude gives NaN for both outputs.  Latitudes are
 * NOT range-checked here (the southern variant holds for [-90, 0]; the Python layer refuses anything else).  points_out may be points_in
 * (in place).  Asynchronous with DBM_DEVICE_PTRS.  Refused (status 1, nothing launched or written): ncol < 2, n >= 2^31, a, 1/f not
 * finite or a <= 0 or 1/f <= 1, a latitude of true scale outside [-90, 0), other parameters not finite, NULL tables with n > 0.
 *
 * dbm_points_region (data_prep.py:353-378 with `gmt info -I<inc>`, NOT `-Is<inc>`): over the rows whose x, y (and z, if ncol >= 3) are
 * all finite, region_out = {floor(xmin / inc) inc, ceil(xmax / inc) inc, floor(ymin / inc) inc, ceil(ymax / inc) inc} and *count_out =
 * the number of such rows (int64); none: four NaNs and 0.  No float atomics, the launch depends on n only: the same bits from call to
 * call.  With DBM_DEVICE_PTRS points, region_out and count_out are device pointers (asynchronous).  Refused (status 1, nothing
 * written): ncol < 2, n >= 2^31, an increment that is not positive and finite, NULL outputs, a NULL table with n > 0.
 *
 * dbm_points_blockmedian (data_prep.py:406-407, `gmt.blockmedian(table, region, spacing="<inc>+e")`, GMT's defaults: gridline
 * registration, no -Q): points is (n, 3) x, y, z.  Grid: region = {xmin, xmax, ymin, ymax}, W = llrint((xmax - xmin) / inc) + 1,
 * H = llrint((ymax - ymin) / inc) + 1 blocks centred on nodes (the north / east edge fitted to the increment, `+e`), row 0 the NORTH
 * row: GridGeometry(x0 = xmin, y0 = ymax, dx = inc, dy = -inc, gridline).  A row with a non-finite x, y or z is dropped
 * (data_prep.py:304); col = floor((x - xmin) / inc + 0.5), row = floor((ymax - y) / inc + 0.5) in float64, IEEE division, no fused
 * multiply-add; the point is used iff 0 <= col < W and 0 <= row < H (so points up to half a block outside the region count); a
 * coordinate exactly on a block boundary goes to the eastern / southern block (this project's choice).  Per non-empty block: the medians
 * of x, of y and of z, each on its own; k values: the middle one, or 0.5 (lo + hi) of the two middle ones, in the total order that puts
 * -0.0 before +0.0.  table_out (table_capacity rows of 3 doubles; host or, with DBM_DEVICE_PTRS, device) receives the m non-empty
 * blocks in block-index order (north row first, west to east: the order blockmedian prints); *n_blocks_out (ALWAYS a host pointer)
 * = m.  grid_dev (H W float32, ALWAYS device, may be NULL): median z rounded to float32 once, NaN in empty blocks; counts_dev (H W
 * int32, ALWAYS device, may be NULL): points per block.  Every output is a function of the multiset of rows: the same bytes from call to
 * call and under any permutation of the rows (integer atomics for the histogram and the placement only, no float atomics).  The call
 * reads m back before it writes anything, so it synchronises the context's stream once even with DBM_DEVICE_PTRS.  min(n, H W) rows
 * of capacity always suffice.  Refused (status 1, no output written): n >= 2^31, H W >= 2^31, a spacing that is not positive and
 * finite, a region that is not finite or has max < min, NULL region / n_blocks_out / table_out (with capacity > 0) / points (n > 0),
 * table_capacity < m. */
int dbm_points_polar_stereographic(dbm_ctx* ctx, const double* points_in, size_t n, int ncol, const double proj[6], double* points_out,
                                   int flags);
int dbm_points_region(dbm_ctx* ctx, const double* points, size_t n, int ncol, double increment, double* region_out, int64_t* count_out,
                      int flags);
int dbm_points_blockmedian(dbm_ctx* ctx, const double* points, size_t n, const double region[4], double spacing, double* table_out,
                           size_t table_capacity, int64_t* n_blocks_out, float* grid_dev, int* counts_dev, int flags);

/* ---- from block medians to the 250 m raster: the second half of xyz_to_grid (data_prep.py:410-419 `gmt.surface(T=0.35, M="3c")`,
 * :420-441 `grdsample -T`) ----
 * dbm_grid_tension_surface (data_prep.py:410-419).  data_dev: float32 (H, W), device, square cells; NaN = free node, any other value =
 * constraint (what dbm_points_blockmedian writes to grid_dev).  out_dev (H, W, device) = the unique minimiser u, with u = data on the
 * constraint nodes, of
 *     E(u) = (1 - T) (sum sxx^2 + sum syy^2 + 2 sum sxy^2) + T (sum sx^2 + sum sy^2),   T = tension,
 * sxx[r, c] = u[r, c-1] - 2 u[r, c] + u[r, c+1] for 1 <= c <= W-2, syy the same along rows, sxy[r, c] = u[r+1, c+1] - u[r+1, c] -
 * u[r, c+1] + u[r, c] for r <= H-2, c <= W-2, sx, sy the first differences.  A difference whose stencil does not fit inside the grid does
 * not exist: that is the whole boundary condition (the plate's natural free edge, no ghost rows).  In the interior the Euler equation is
 * GMT's, (1 - T) del^4 u - T del^2 u = 0 (at T = 0.35: 14.4 at the node, -5.55 at the four neighbours, 1.3 at the diagonals, 0.65 at
 * distance two).  Solved in float64: the data are shifted by the value m of the constraint node with the lowest row-major index,
 * A_FF x = b = -[A (d - m on constraints, 0 elsewhere)]_F by Jacobi-preconditioned conjugate gradients from x = 0 until |r| <= tol |b|
 * (the recursively updated residual; b = 0: zero iterations, no division), u = x + m on free nodes, rounded to float32 once; constraint
 * nodes are copied bit for bit.  No float atomics, launch shapes depend on H and W only: the same bytes from call to call.  The residual
 * is read back every 32 iterations; the iterations stop on the device at the one that converged.  info (HOST, 4 doubles) =
 * {iterations, final |r| / |b| (0 for b = 0), constraint nodes, free nodes}.  The call allocates its workspace (33 bytes per node),
 * frees it on every path, and synchronises.
 * DIFFERENT FROM GMT `surface`: constraints sit ON nodes (a block median's sub-cell offset is ignored: no Briggs off-node
 * terms); natural boundary rows instead of GMT's edge conditions; no plane detrending, only the constant shift; a residual stopping rule
 * instead of GMT's per-node change limit; no multigrid schedule (it changes the path, not the minimiser).  Results differ from GMT's
 * wherever data do not sit on nodes; the reference's nine-number doctest (data_prep.py:393-404) is not reproduced.
 * Status 1 (refused, nothing written): H or W < 3, H W >= 2^31, tension outside (0, 1] (T = 0 needs three non-collinear constraints
 * and is left out), tol outside (0, 1), max_iter outside 1..10^6, NULL pointers, no constraint node (found by one counting launch).
 * Status 10: not converged within max_iter; out_dev holds the last iterate and info is filled.
 *
 * dbm_grid_distance_mask (`M="3c"`): grid_dev[r, c] (device, in place) becomes NaN unless some non-NaN node (r', c') of data_dev has
 * (r - r')^2 + (c - c')^2 <= radius^2 (integers).  The Euclidean node-to-node distance is this project's reading of GMT's `c` unit
 * (cells); GMT measures from the data POINTS, which sit up to half a cell from their nodes.  Asynchronous.  Status 1: radius outside
 * 0..32, grid_dev == data_dev, NULL pointers, H W outside 1..2^31 - 1.
 *
 * dbm_grid_to_pixel (`grdsample -T`, data_prep.py:420-441): out_dev (H - 1, W - 1) = dbm_grid_track's bicubic interpolant (same Keys
 * weights, linear ghost nodes, NaN nodes and threshold rule) of in_dev (H, W) at the cell centres, node coordinates (c + 1/2, r + 1/2),
 * rounded to float32 once: the gridline-registered grid becomes the pixel-registered grid of the same region, node (0, 0) at
 * (x0 + dx / 2, y0 + dy / 2).  Asynchronous.  Status 1: H or W < 2, H W >= 2^31, threshold outside (0, 1], out_dev == in_dev, NULL. */
int dbm_grid_tension_surface(dbm_ctx* ctx, const float* data_dev, long H, long W, double tension, double tol, int max_iter,
                             float* out_dev, double info[4]);
int dbm_grid_distance_mask(dbm_ctx* ctx, const float* data_dev, float* grid_dev, long H, long W, int radius);
int dbm_grid_to_pixel(dbm_ctx* ctx, const float* in_dev, long H, long W, double threshold, float* out_dev);

/* ---- tiles inside the buffered grounding line (data_prep.py:582-616, "Subset tiles to those within grounding line":
 * `gline.geometry.buffer(distance=10000)` at :602, `gpd.sjoin(tile_gdf, op="within", gline)` at :606) ----
 * dbm_grid_polygon_mask marks the nodes of a raster that lie inside a polygon set dilated (buffer >= 0) or eroded (buffer < 0) by
 * |buffer|.  It is this project's own, exactly defined selection, NOT a reproduction of GEOS: GEOS replaces the arcs of
 * the offset curve by polygons (8 segments per quadrant: up to 10 000 (1 - cos(pi / 32)) ~ 48 m inside the true 10 km offset) and tests
 * boxes, not nodes.
 * Polygon set: edges is (n_edges, 4) float64 rows (xa, ya, xb, yb), C-contiguous -- ALL rings of ALL parts pooled, holes included, each
 * ring closed (the last vertex joined to the first); a host table, or with DBM_DEVICE_PTRS a device table (16-byte aligned).
 * Node (r, c) sits at x = x0 + c dx, y = y0 + r dy, geom = {x0, y0, dx, dy} as dbm_grid_tile takes it: one multiplication and one
 * addition, each rounded.  All arithmetic is float64 IEEE, no fused multiply-add, IEEE division.
 * Inside: the even-odd rule over all edges.  An edge counts iff (ya <= y) != (yb <= y) and x < xa + ((y - ya) * (xb - xa)) / (yb - ya);
 * inside = the count is odd.  Ring orientation therefore does not matter, a hole is simply another ring, and where two parts overlap
 * they CANCEL (the overlap is outside) -- unlike a union.  Horizontal edges never count.
 * Distance: ex = xb - xa, ey = yb - ya, px = x - xa, py = y - ya, L = ex ex + ey ey; t = L > 0 ? (px ex + py ey) / L : 0, clamped to
 * [0, 1]; qx = px - t ex, qy = py - t ey, d2 = qx qx + qy qy; near = some edge has d2 <= buffer * buffer.
 * Mask: buffer >= 0 (-0.0 included): inside || near -- the closed Euclidean dilation with round joins, boundary nodes are in;
 * buffer < 0: inside && !near -- the erosion.  No edges: 0 everywhere.
 * mask_dev (H W bytes of 0 / 1, ALWAYS device, may be NULL); grid_dev (H W float32, ALWAYS device, may be NULL): changed in place, NaN
 * where the mask is 0, every other node's bits untouched; at least one of the two.  Tile selection (data_prep.py:606) is then
 * dbm_grid_filled_windows on that raster: a window is kept iff every one of its nodes is in the mask and holds data.
 * Both results are order-independent (a parity and an "any"): the same bytes from call to call, under any permutation of the edges, and on
 * either schedule -- edges binned per tile of DBM_POLY_TILE^2 nodes, or, when the bins would take more than workspace_limit bytes (0: a
 * default of 256 MiB), every tile running over the culled lists.  Culling never changes a result: boxes are grown by |buffer| plus a
 * margin of 2^-30 of the coordinate magnitude, far above the rounding of d2 (polygon.hip).  Integer atomics place list entries; no float
 * atomics.  The call allocates its workspace (about 8 bytes per edge, 12 per node tile, 4 per bin entry; 32 per edge more for a host
 * table), frees it on every path, and synchronises the context's stream: once to read the list sizes back (and, for a device table,
 * whether a coordinate was not finite -- before anything is written) and once before the workspace is released.
 * Relation to the reference: a box within the true dilation has all its nodes in it, so this selection CONTAINS the true one; the two
 * differ only for windows where the offset curve passes within half a pixel diagonal of the window's box (177 m at 250 m pixels), the
 * same order as GEOS's own 48 m.  The reference's 4028-tile list cannot be reproduced without its shapefile; nothing is claimed about it.
 * Refused (status 1, nothing written): NULL ctx or geom, H or W < 1, H W >= 2^31, n_edges >= 2^31, geom not finite or dx or dy zero,
 * buffer not finite, a non-finite edge coordinate, both outputs NULL, NULL edges with n_edges > 0.
 * dbm_grid_polygon_stats: out (HOST) = {proximity edges kept by the cull, parity edges kept, tile bin entries, band bin entries,
 * schedule (0 unbinned, 1 binned, 2 no culling: a coordinate beyond 2^480), n_edges} of the context's last successful call. */
int dbm_grid_polygon_mask(dbm_ctx* ctx, const double* edges, size_t n_edges, long H, long W, const double geom[4], double buffer,
                          unsigned char* mask_dev, float* grid_dev, size_t workspace_limit, int flags);
int dbm_grid_polygon_stats(dbm_ctx* ctx, int64_t out[6]);

/* ---- the maps' vector layers (paper_figures.py:533-562, Figure 2: `fig.coast(shorelines="0.25p")` -- the grounding line on the DEM --
 * and `fig.plot(style="r+s", pen="1p,orange2")` -- the study regions and the training tiles as boxes; paper_figures.py:1039-1045, Figure
 * 5a: `fig.plot(style="c0.1c", color="orange")` -- the transect's survey points on the Thwaites DEM) ----
 * dbm_image_overlay paints ONE layer -- primitives of one kind, one size in pixels and one colour -- onto a resident image, in place.
 * It is this project's own, exactly defined rule, NOT GMT's pixels (deepbedmap_amd/overlay.py: draw_layers_host is its
 * NumPy statement).
 * image_dev: uint8 (H, W, channels), channels 3 or 4, C-contiguous, ALWAYS device.  geom = {x0, y0, dx, dy}: pixel (r, c) has its
 * centre at (x0 + c dx, y0 + r dy); either sign of dx and dy.
 * prims: n rows of `stride` float64, a host table, or with DBM_DEVICE_PTRS a device table.  kind DBM_OVERLAY_SEGMENTS: rows (xa, ya,
 * xb, yb), stride 4, drawn with a pen of size_px pixels; a segment of length zero is a dot.  kind DBM_OVERLAY_DISCS: rows (x, y) or
 * (x, y, z) -- stride 2 or 3, z is not read -- drawn as discs of diameter size_px pixels.
 * 1. Pixel units: u = (x - x0) / dx, v = (y - y0) / dy: one float64 subtraction and one division, each rounded.  All arithmetic below
 *    is float64 IEEE, no fused multiply-add, IEEE division.
 * 2. Pixel (r, c) has samples x samples sub-samples, samples S in {1, 2, 4}; sub-sample (i, j) lies at su = c + ((j + 1/2) / S - 1/2),
 *    sv = r + ((i + 1/2) / S - 1/2), exactly.
 * 3. With h = size_px / 2 and h2 = h * h (rounded once), a sub-sample is covered if SOME primitive has d2 <= h2 (closed).  Segments:
 *    ex = ub - ua, ey = vb - va, px = su - ua, py = sv - va, L = ex ex + ey ey; t = L > 0 ? (px ex + py ey) / L : 0, clamped to [0, 1];
 *    qx = px - t ex, qy = py - t ey, d2 = qx qx + qy qy -- dbm_grid_polygon_mask's distance in pixel units.  Discs: px = su - u,
 *    py = sv - v, d2 = px px + py py.  A primitive whose pixel coordinates overflow covers nothing (d2 is inf or NaN).
 * 4. With m = the number of covered sub-samples of the pixel, A = rgba[3], w = m A and D = S S 255, every colour channel becomes
 *    (w rgba[ch] + (D - w) dst + D / 2) / D in integers (floor division); a fourth channel by the same formula with 255 in the place of
 *    rgba[ch].  A pixel with m = 0 is not written.
 * Layers are painted by successive calls, each over the result of the one before.
 * The result is order-independent (an "any"): the same bytes from call to call, under any permutation of the primitives, and on either
 * schedule -- primitives binned per tile of DBM_OVERLAY_TILE^2 pixels, or, when the bins would take more than workspace_limit bytes (0: a
 * default of 256 MiB), every tile running over the whole list of kept primitives.  Culling never changes a result: boxes are grown by
 * the radius plus a margin of 2^-30 of the coordinate magnitude, far above the rounding of d2 (overlay.hip).  Integer atomics place list
 * entries; no float atomics.  Pixels are indexed with 64-bit integers: an image may hold more than 2^31 bytes.  The call allocates its
 * workspace (32 bytes per segment, 16 per disc, 12 per pixel tile, 4 per bin entry; 8 stride per primitive more for a host table), frees
 * it on every path, and synchronises the context's stream: once to read the counters back (for a device table, whether a coordinate was
 * not finite -- before anything is written) and once before the workspace is released.
 * Refused (status 1, nothing written): NULL ctx, image, geom or rgba, H or W < 1, H W >= 2^31, channels not 3 or 4, n >= 2^31, geom not
 * finite or dx or dy zero, a kind that is neither, stride not 4 for segments or not 2 or 3 for discs, size_px negative or not finite,
 * samples not 1, 2 or 4, a non-finite x or y of a primitive, NULL prims with n > 0.
 * dbm_image_overlay_stats: out (HOST) = {primitives kept by the cull, tile bin entries, schedule (0 unbinned, 1 binned), n} of the
 * context's last successful call. */
int dbm_image_overlay(dbm_ctx* ctx, unsigned char* image_dev, long H, long W, int channels, const double geom[4], const double* prims,
                      size_t n, int kind, int stride, double size_px, const unsigned char rgba[4], int samples, size_t workspace_limit,
                      int flags);
int dbm_image_overlay_stats(dbm_ctx* ctx, int64_t out[4]);

/* ---- optimizer ---- */
/* chainer.optimizers.Adam(alpha, eps=1e-8).setup(model): srgan_train.py:1043-1048 */
int dbm_adam_setup(dbm_model* m, double alpha, double beta1, double beta2, double eps);
/* optimizer.update(): srgan_train.py:1164, 1257.  grad_scale multiplies the gradient first (1/world after a
 * sum all-reduce). */
int dbm_adam_update(dbm_model* m, double grad_scale);

/* Whole-arena gradient all-reduce on the context's stream for callers that drive dbm_gen_backward / dbm_disc_backward
 * themselves (no overlap); *grad_scale (may be NULL) receives 1 / world for dbm_adam_update. */
int dbm_allreduce_grads(dbm_model* m, double* grad_scale);

/* ---- fused steps (device-resident inputs, asynchronous) ---- */
/* train_eval_discriminator: srgan_train.py:1084-1166 up to and including d_loss.backward() (update = dbm_adam_update).
 * arrays are DEVICE pointers: X (N,1,11,11), W1 (N,1,110,110), W2 (N,2,22,22), W3 (N,1,11,11), Y (N,1,36,36).
 * metrics_dev (device, >= 8 floats) receives [d_loss, d_accu].
 * train: bit 0 = training mode (0 evaluates with BatchNorm in eval mode); scheduling options, all numerically neutral:
 * bit 1 (2) = keep this call's generator forward for the following dbm_generator_step on the same arrays (that step
 * then skips its own forward: NOT what the reference does, off by default); bit 2 (4) = the following
 * dbm_generator_step's forward is enqueued now, in its own workspace and on separate streams, underneath this
 * step's discriminator passes (the trainer's pattern; discarded if the next call does not match); bit 3 (8) = the
 * caller runs collectives on a stream of its own: the prefetched forward stays on one library stream; bit 4 (16) = do
 * not exchange gradients inside the call although the context has a communicator (dbm_comm_init). */
int dbm_discriminator_step(dbm_model* g, dbm_model* d, int N, int H, int W, const float* X, const float* W1,
                           const float* W2, const float* W3, const float* Y, int train, float* metrics_dev);
/* train_eval_generator: srgan_train.py:1170-1263 up to and including g_loss.backward().
 * metrics_dev receives [., ., g_loss, psnr, ssim].
 * train: bit 0 = training mode; bit 1 (2) = reuse the generator forward the preceding dbm_discriminator_step kept
 * (its bit 1); bit 2 (4) = consume the forward that step prefetched (its bit 2): the caller asserts that the five
 * arrays are the same, UNCHANGED, device arrays.  The library additionally checks pointers, shapes, the parameter
 * version and its own record of writes to device memory (dbm_memcpy_h2d, dbm_gather_rows, dbm_fill_f32,
 * dbm_memcpy2d_d2d, dbm_grid_tile, dbm_grid_filled_windows, dbm_grid_fill_gaps, dbm_tiff_decode, dbm_chunk_decode, dbm_grid_rescale, dbm_grid_rolling_std, dbm_malloc, dbm_free); writes by anybody else (another library filling the same buffer in
 * place) are invisible to it, hence the explicit bit.  Without it the prefetched pass is discarded and the forward is
 * recomputed.  bit 4 (16) = see dbm_discriminator_step. */
int dbm_generator_step(dbm_model* g, dbm_model* d, int N, int H, int W, const float* X, const float* W1,
                       const float* W2, const float* W3, const float* Y, const float weights[4], int ssim_window,
                       int train, float* metrics_dev);

/* ---- output format of the DEM (deepbedmap.py:749-756: `save_array_to_grid(array=Y_hat.astype(np.int16), dtype=np.int16,
 * tiled=True, compression=lzw)` -> data_prep.py:779-834, a tiled LZW GeoTIFF written by rasterio / GDAL) ----
 * dbm_f32_to_i16: `Y_hat.astype(np.int16)` on the device canvas (NumPy's cast: truncation, NaN / inf / out of range -> 0),
 * asynchronous on the context's stream; dst_dev holds n int16 values.
 * dbm_lzw_encode_tiles: TIFF 6.0 LZW of `ntiles` tiles of `tile_bytes` bytes each (host memory, tile t at
 * tiles + t * tile_bytes) into out + t * out_stride (out_stride >= tile_bytes * 3 / 2 + 64 is always enough),
 * encoded sizes in out_sizes[t]; tiles are spread over `nthreads` host threads.  dbm_lzw_decode: one stream back
 * (round-trip check).  dbm_inflate: one zlib stream (RFC 1950 around RFC 1951, dbm_tiff_decode's compression 8) decoded on the host
 * by the device decoder's own loop run with one lane; *out_bytes = the decoded size; non-zero on everything that decoder reports (a
 * malformed stream, more than cap bytes of output).  Host functions: no GPU, no context.  The TIFF container is written by the host
 * shim (deepbedmap_amd/geotiff.py).
 * dbm_deflate_encode_blocks: `nblocks` blocks of `block_bytes` bytes each (host memory, block t at blocks + t * block_bytes), each as one
 * zlib stream -- header 78 01, one final block with the fixed Huffman code, the Adler-32 -- by the matching rule of dbm_chunk_encode
 * (the device encoder's own loop run with one lane: the bytes are the device's), into out + t * out_stride (out_stride >= block_bytes +
 * block_bytes / 8 + 16 is always enough), sizes in out_sizes[t]; blocks are spread over `nthreads` host threads.  Status 2: a stream did
 * not fit out_stride. */
int dbm_f32_to_i16(dbm_ctx* ctx, const float* src_dev, void* dst_dev, size_t n);
int dbm_lzw_encode_tiles(const void* tiles, size_t tile_bytes, int ntiles, void* out, size_t out_stride, size_t* out_sizes,
                         int nthreads);
int dbm_lzw_decode(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes);
int dbm_inflate(const void* src, size_t nbytes, void* dst, size_t cap, size_t* out_bytes);
int dbm_deflate_encode_blocks(const void* blocks, size_t block_bytes, int nblocks, void* out, size_t out_stride, size_t* out_sizes,
                              int nthreads);

/* ---- opening rasters: GeoTIFF blocks decoded on the device (replaces the rasterio / GDAL reads of data_prep.py:668, :845-877 and
 * deepbedmap.py:164-204; header parsing, the block plan and file reads stay with the host shim deepbedmap_amd/geotiff.py) ----
 * dbm_tiff_decode turns n_blocks blocks (strips or tiles) of one-sample pixels into their places of the float32 plane out_dev (out_h,
 * out_w), ALWAYS a device pointer.  streams_host (streams_bytes bytes, HOST, uploaded once per call) holds the blocks' bytes;
 * blocks_host (HOST) has 8 int64 per block: {offset of its bytes in streams_host, their count, rows the block holds (1..block_h: the
 * last strip is short, tiles are whole), output row of the block's row 0, output column of its column 0 (either may be negative or
 * beyond the plane: samples outside [0, out_h) x [0, out_w) are dropped -- tile padding, the part outside a window), id (only named
 * in error messages), 0, 0}.  A block row has block_w samples.
 * compression 5: the bytes are a TIFF 6.0 LZW stream (MSB-first codes, 9..12 bits, early change, ClearCode 256, EndOfInformation 257:
 * what dbm_lzw_decode reads), decoded by one wavefront per block; a stream may end without EndOfInformation if the block is complete.
 * compression 8: the bytes are a zlib stream (RFC 1950: CM 8, CINFO <= 7, header check, no preset dictionary; RFC 1951 inside: stored,
 * fixed and dynamic blocks; the Adler-32 of the decoded bytes behind it, bytes after that ignored), accepted and refused as zlib's
 * `uncompress` does it, decoded by one wavefront per block; no alignment or length condition, as for 5.  TIFF Compression 32946 is
 * the same codec: pass 8.
 * compression 1: the bytes ARE the decoded block (uncompressed files; deflate inflated by the caller), offset a multiple of 8, count
 * >= rows * block_w * bytes.
 * predictor (TIFF tag 317) 1: none; 2: every row is a running sum of its samples, wrapping in the sample's width (float samples:
 * on their bit patterns); 3 (float samples): every row's block_w * bytes bytes are a running sum modulo 256, then byte plane k
 * (block_w bytes) holds byte k of every sample, most significant first.
 * sample_type 0 uint8, 1 int16, 2 uint16, 3 int32, 4 float32, 5 float64, little endian; converted as numpy.astype(float32) does
 * (float32 samples keep their bits, NaN payloads included).
 * The call allocates its workspace (streams_bytes + 68 per block; for LZW and deflate also block_w * block_h * bytes, rounded up to 16, per
 * block), frees it on every path and synchronises the context's stream; the caller bounds the workspace by batching.
 * Status 11: an LZW stream is malformed (a first code above 255, a code above the next free one, more output than the block holds) or
 * does not decode to rows * block_w * bytes bytes; or a deflate stream is malformed (a bad zlib header or a preset dictionary, block
 * type 3, a stored block whose NLEN is not ~LEN or that is longer than the stream, HLIT > 286 or HDIST > 30, a repeat code with no
 * previous length or past the last one, no end-of-block code, an over-subscribed or incomplete set of code lengths -- but a single
 * code of length 1 and no distance code at all pass, as in zlib --, a bit pattern that is no code, symbols 286 / 287, distance codes
 * 30 / 31, a distance beyond what has been written, more output than the block holds, a stream that ends early, an Adler-32 that does
 * not match) or does not decode to that size; the message names the block's id and nothing of this call has been written.
 * Refused (status 1, nothing launched): compression not 1, 5 or 8, sample_type outside 0..5, predictor not 1, 2 or 3 (3: float samples
 * only), block_w or block_h < 1, a block of 2^31 bytes or more, n_blocks * block_h >= 2^31, an empty plane, NULL pointers with
 * n_blocks > 0, bytes outside streams_host, rows outside 1..block_h, decoded bytes misaligned or short.  n_blocks = 0 succeeds. */
int dbm_tiff_decode(dbm_ctx* ctx, const void* streams_host, size_t streams_bytes, const int64_t* blocks_host, int n_blocks, int compression,
                    int predictor, int sample_type, int block_w, int block_h, float* out_dev, long out_h, long out_w);

/* ---- opening netCDF grids: chunks and row bands placed on the device (replaces the xarray / rasterio reads of netCDF files: the ice
 * velocity `netcdf:misc/antarctic_ice_vel_phase_map_v01.nc:VX` / `:VY` of data_prep.py:889-900 and deepbedmap.py:176-191, the ground-truth
 * grids of deepbedmap.py:74-78; the HDF5 / classic container, the chunk plan and file reads stay with the host shim
 * deepbedmap_amd/netcdf.py) ----
 * dbm_chunk_decode turns n_blocks blocks (HDF5 chunks, or row bands of contiguous / classic data: blocks with block_w == the variable's
 * width) into their places of the float32 plane out_dev (out_h, out_w), ALWAYS a device pointer.  streams_host / streams_bytes /
 * blocks_host as for dbm_tiff_decode, with a row step: 8 int64 per block, {offset of its bytes, their count, rows held (1..block_h),
 * output row of the block's row 0, output column of its column 0, id (only named in error messages), row step (+1 or -1), 0}.  Row r
 * of a block lands on output row e[3] + step * r (step -1: a file whose rows run south to north is returned north-up); samples outside
 * [0, out_h) x [0, out_w) are dropped (the columns of edge chunks beyond the dataset, the part of a chunk outside a window); cells no
 * block covers keep what they held.
 * compression 8: the bytes are a zlib stream (dbm_tiff_decode's compression 8, the same decoder: one wavefront per block) that decodes
 * to exactly block_h * block_w * bytes bytes -- an HDF5 chunk is always stored whole, whatever `rows held` says.  compression 1: the
 * bytes ARE the block, offset a multiple of 8, count >= rows held * block_w * bytes (shuffle 1: >= block_h * block_w * bytes).
 * shuffle 1: HDF5's shuffle filter over the WHOLE block of n = block_h * block_w elements is undone: byte k of element i lies at
 * k * n + i.  big_endian 1: the samples are stored most significant byte first.
 * sample_type: dbm_tiff_decode's 0 uint8, 1 int16, 2 uint16, 3 int32, 4 float32, 5 float64, and 6 int8.
 * Values: has_fill 1: a sample that equals the fill (fill_bits: the fill's bits in the sample's width, native order, upper bits 0) BY
 * VALUE in its stored type becomes NaN (floats: -0.0 equals 0.0, a NaN fill matches every NaN).  has_scale 1: every other sample
 * becomes float32(float64(v) * scale + offset), two separately rounded float64 operations (never an FMA) and one rounding to float32;
 * has_scale 0: numpy.astype(float32) (float32 samples keep their bits, NaN payloads included).
 * The call allocates its workspace (streams_bytes + 68 per block; for compression 8 also 64 bytes and block_w * block_h * bytes,
 * rounded up to 16, per block), frees it on every path and synchronises the context's stream; the caller bounds it by batching.
 * Status 11: a zlib stream is malformed (dbm_tiff_decode's list) or does not decode to exactly block_h * block_w * bytes bytes; the
 * message names the block's id and nothing of this call has been written.
 * Refused (status 1, nothing launched): compression not 1 or 8, shuffle, big_endian, has_fill or has_scale not 0 or 1, sample_type
 * outside 0..6, fill_bits wider than the sample, block_w or block_h < 1, a block of 2^31 bytes or more, 2^31 workgroups or more
 * (n_blocks * ceil(block_h * block_w / 1024)), an empty plane, NULL pointers with n_blocks > 0, bytes outside streams_host, rows
 * outside 1..block_h, a row step other than +1 / -1, decoded bytes misaligned or short, a placement beyond +-2^40.  n_blocks = 0
 * succeeds. */
int dbm_chunk_decode(dbm_ctx* ctx, const void* streams_host, size_t streams_bytes, const int64_t* blocks_host, int n_blocks, int compression,
                     int shuffle, int sample_type, int big_endian, int block_w, int block_h, int has_fill, uint64_t fill_bits, int has_scale,
                     double scale, double offset, float* out_dev, long out_h, long out_w);

/* ---- writing the DEM from HBM: GeoTIFF blocks encoded on the device (deepbedmap.py:749-756: `save_array_to_grid(array=
 * Y_hat.astype(np.int16), dtype=np.int16, tiled=True, compression=lzw)` -> data_prep.py:779-834, a tiled LZW GeoTIFF written by rasterio
 * / GDAL; the container, its tags and the batching stay with the host shim deepbedmap_amd/geotiff.py: write_geotiff_resident) ----
 * dbm_tiff_encode turns blocks first .. first + n_blocks - 1 (row-major over the image's blocks) of the float32 plane plane_dev (H, W),
 * ALWAYS a device pointer, into their bytes as a TIFF holds them and downloads only those.
 * sample_type (dbm_tiff_decode's numbering) 1: int16 by the cast of dbm_f32_to_i16 (NumPy's astype: truncation, NaN / inf / |x| >= 2^31
 * -> 0); 4: float32, the bits (NaN payloads kept).  Little endian.
 * tiled != 0: blocks of block_h x block_w are whole, positions right of or below the plane are zero bytes; tiled == 0: strips,
 * block_w == W, the last strip holds only the rows that exist.
 * predictor (TIFF tag 317) 1: none; 2: horizontal differencing per block row in the sample's own width, wrapping (int16: on uint16;
 * float32: on the 32-bit patterns): d[0] = s[0], d[c] = s[c] - s[c - 1] over the block's row including its padding columns -- the
 * inverse of what dbm_tiff_decode undoes.
 * compression 5: every block becomes a TIFF 6.0 LZW stream, byte for byte the one dbm_lzw_encode_tiles writes for the same bytes,
 * encoded by one wavefront per block; compression 1: the bytes themselves (predictor applied as asked: the caller decides).
 * out_host (HOST, out_capacity bytes) receives the blocks one behind the other, each at the next even offset from 0 (an odd block is
 * followed by one zero byte); sizes_host (HOST) the n_blocks sizes.  out_capacity must cover the worst case: n_blocks times
 * block_h * block_w * bytes * 3 / 2 + 64 (compression 5) or block_h * block_w * bytes (compression 1), each rounded up to even.
 * The call allocates its workspace (per block: the raw block rounded up to 16, 24 bytes of bookkeeping, for LZW the slot of the worst
 * case; plus the packed streams), frees it on every path and synchronises the context's stream; the caller bounds it by batching.
 * Status 12: a block's LZW stream did not fit its slot; the message names the block and nothing of this call was written.  It cannot
 * occur with the slot above (incompressible bytes grow by a factor of about 1.41) and is there as the guard of the device loop.
 * Refused (status 1, nothing launched): NULL pointers, an empty plane or H * W >= 2^31, sample_type not 1 or 4, compression not 1 or 5,
 * predictor not 1 or 2, block_w or block_h < 1, a block of 2^31 bytes or more, strips that are not W wide, a block range outside the
 * image, n_blocks * block_h >= 2^31, out_capacity below the worst case.  n_blocks = 0 succeeds. */
int dbm_tiff_encode(dbm_ctx* ctx, const float* plane_dev, long H, long W, int sample_type, int block_h, int block_w, int tiled, int predictor,
                    int compression, long first, int n_blocks, void* out_host, size_t out_capacity, size_t* sizes_host);

/* ---- writing grids as netCDF-4 from HBM: chunks cut, shuffled and deflated on the device (data_prep.py:826-830: `save_array_to_grid(
 * save_netcdf=True)`, the model's deepbedmap3.nc / elevdiffmap.nc of deepbedmap.py:425-437; data_prep.py:410-441: `xyz_to_grid(outfile=
 * ...)`, the chunked, deflated highres grids GMT writes; the HDF5 container and the batching stay with the host shim
 * deepbedmap_amd/netcdf.py: write_netcdf_resident) ----
 * dbm_chunk_encode turns chunks first .. first + n_blocks - 1 (row-major over the variable's chunks of chunk_h x chunk_w) of the float32
 * plane plane_dev (H, W), ALWAYS a device pointer, into the bytes an HDF5 file stores for them and downloads only those.
 * Row r of the chunk whose first row is r0 is plane row r0 + r (row_step +1) or H - 1 - (r0 + r) (row_step -1: a file whose y ascends;
 * the inverse of dbm_chunk_decode's row step).  Chunks are whole: positions beyond the plane are zero bytes.  The values are the 32-bit
 * patterns, little endian (NaN payloads and -0.0 kept).  shuffle 1: HDF5's shuffle filter over the whole chunk of n = chunk_h * chunk_w
 * elements: byte k of element i goes to k * n + i.
 * compression 8: every chunk becomes one zlib stream (RFC 1950 around RFC 1951): header 78 01, ONE final block with the fixed Huffman
 * code, the Adler-32; greedy matches of 3..258 bytes at distances 1..32768 from a 16 384-entry hash table (the rule: DESIGN.md 6m), one
 * wavefront per chunk, byte for byte the stream dbm_deflate_encode_blocks writes for the same bytes.  compression 1: the bytes themselves.
 * out_host (HOST, out_capacity bytes) receives the chunks one behind the other, each at the next even offset from 0 (an odd stream is
 * followed by one zero byte); sizes_host (HOST) the n_blocks sizes.  out_capacity must cover the worst case: n_blocks times
 * chunk_bytes + chunk_bytes / 8 + 16 (compression 8: no input byte costs more than 9 bits) or chunk_bytes (compression 1), each
 * rounded up to even, chunk_bytes = chunk_h * chunk_w * 4.
 * The call allocates its workspace (per chunk: the raw chunk rounded up to 16, 24 bytes of bookkeeping, for deflate the slot of the worst
 * case; plus the packed streams), frees it on every path, synchronises the context's stream, writes no caller-visible device memory and
 * reads no environment variable; the caller bounds the workspace by batching.
 * Status 12: a chunk's deflate stream did not fit its slot; the message names the chunk and nothing of this call was written.  It cannot
 * occur with the slot above and is there as the guard of the device loop.
 * Refused (status 1, nothing launched): NULL pointers, an empty plane or H * W >= 2^31, compression not 1 or 8, shuffle not 0 or 1, a row
 * step other than +1 / -1, chunk_h or chunk_w < 1 or larger than H or W, a chunk of 2^31 bytes or more, a chunk range outside the image,
 * 2^31 workgroups or more (n_blocks * ceil(chunk_h * chunk_w / 1024)), out_capacity below the worst case.  n_blocks = 0 succeeds. */
int dbm_chunk_encode(dbm_ctx* ctx, const float* plane_dev, long H, long W, int chunk_h, int chunk_w, int row_step, int shuffle, int compression,
                     long first, int n_blocks, void* out_host, size_t out_capacity, size_t* sizes_host);

/* ---- the overviews of that file, built next to the canvas (deepbedmap.py:749-756 -> data_prep.py:779-834 write one full-resolution
 * image; its readers then run `gdaladdo -r average`.  The directories and the container stay with deepbedmap_amd/geotiff.py) ----
 * dbm_grid_overviews halves the float32 plane plane_dev (H, W) `levels` times and writes the levels back to back to out_dev as float32
 * planes of ceil(H / 2) x ceil(W / 2), ceil(H / 4) x ceil(W / 4), ...; both are DEVICE pointers and the call only enqueues.
 * sample_type (dbm_tiff_encode's) 1: level 0 is the int16 cast of the plane (the canvas itself is not touched), every result is rounded
 * to even and stored as an exactly representable float, so that dbm_tiff_encode encodes a level unchanged; 4: float32.
 * Level k + 1 is made from level k alone: pixel (r, c) is the mean of the samples of rows 2r, 2r + 1 and columns 2c, 2c + 1 that exist
 * and are valid (float32: neither NaN nor float32(*nodata); int16: not int(*nodata)): s = (a00 + a01) + (a10 + a11) in float32 with
 * +0.0f for the others, divided by their number n in one IEEE division; n == 0 gives float32(*nodata) / int(*nodata).  nodata is a HOST
 * pointer to one value.  Three levels come out of one pass over memory; the results are those of one halving at a time, bit for bit.
 * Refused (status 1, nothing launched): NULL pointers, an empty plane or H * W >= 2^31, sample_type not 1 or 4, a nodata value that is
 * not finite with sample_type 1, levels < 0 or beyond the first 1 x 1 level (the message says how many the plane admits), out_dev ==
 * plane_dev.  levels = 0 succeeds. */
int dbm_grid_overviews(dbm_ctx* ctx, const float* plane_dev, long H, long W, int sample_type, const double* nodata, int levels,
                       float* out_dev);

/* ---- rendering the DEM from HBM: colour relief, hillshade, PNG (deepbedmap.py:758-775: `gmt.makecpt(cmap="oleron", series=[-4500,
 * 4500])`, `fig.grdimage(..., cmap=True, Q=True)`, `fig.savefig("deepbedmap_dem.png")`; paper_figures.py:692-699: the same with
 * `shading="+d"`.  Colour tables, the PNG container and the batching stay with the host shim deepbedmap_amd/relief.py.  The rules are
 * this project's own -- GMT's pixels are not claimed: DESIGN.md 6n) ----
 * dbm_grid_relief (deepbedmap.py:758-775, paper_figures.py:692-699) colours the float32 plane plane_dev (H, W) into out_dev, uint8
 * (H, W, channels), both DEVICE pointers; the call only enqueues.  edges_host (HOST, n_slices + 1 doubles, strictly ascending) and
 * colors_host (HOST, 6 n_slices + 9 bytes: per slice the colour r, g, b at its lower edge and at its upper edge, then the colours B
 * below the table, F above it and N of NaN) are copied up by the call.  Per pixel, v = (double)z, every operation one IEEE float64
 * operation, never an FMA: NaN gives N (alpha 0 with 4 channels; alpha is 255 everywhere else); v < E_0 gives B, v > E_n gives F (so
 * -inf and +inf); else i = the largest index <= n - 1 with E_i <= v, t = (v - E_i) / (E_{i+1} - E_i), u = c0 + (c1 - c0) t per
 * channel (the product rounded, then the sum).  shade != 0: I = k atan((g - mean) / sigma) where the gradient g is defined, else 0; I >= 0:
 * u' = u + (255 - u) I; I < 0: u' = u + u I; B and F pixels are shaded, N pixels are not.  Byte = floor(u' + 0.5) clamped to 0..255.
 * g = -(dx sin_a + (dy aspect) cos_a) with dx = (z[r, c + 1] - z[r, c - 1]) / 2 and dy = (z[r - 1, c] - z[r + 1, c]) / 2 (rows
 * north-up, index units), one-sided (the difference of the two samples that exist, not halved) at the first and last column and row;
 * defined only where the four samples it reads are finite, nowhere if W == 1 or H == 1.  The caller computes sin_a, cos_a of the
 * azimuth (the reference's "+d" is azimuth -45 degrees, amplitude 1) and k = amplitude 2 / pi.
 * Refused (status 1, nothing launched): NULL pointers, an empty plane or H * W >= 2^31, channels not 3 or 4, n_slices outside 1..2048,
 * edges that are not finite or not strictly ascending; with shade: sigma <= 0, a mean, sigma, k, sin_a, cos_a or aspect that is not
 * finite, |k| > 2 / pi.
 * dbm_grid_shade_stats (paper_figures.py:692-699: what `shading="+d"` normalises by) returns out_host[3] = {n, mean, sigma} of the
 * defined g of the plane: mean = sum g / n, sigma = sqrt(sum (g - mean)^2 / (n - 1)), two passes in float64 in a fixed order (the same
 * bits from call to call); n == 0 gives mean 0, n < 2 sigma 0.  The call allocates its workspace, frees it on every path and
 * synchronises.  Refused (status 1): NULL pointers, an empty plane or H * W >= 2^31, sin_a, cos_a or aspect not finite.
 * dbm_png_encode (deepbedmap.py:758-775: `fig.savefig`) turns bands first_band .. first_band + n_bands - 1 of the uint8 image
 * image_dev (H, W, channels; channels 1 grey, 3 RGB, 4 RGBA), ALWAYS a device pointer, into segments of the PNG's zlib stream and
 * downloads only those.  Band b holds rows b band_rows ... (the last band is short): per row one filter-type byte and the W channels
 * filtered bytes (filter 0 None, 1 Sub, 2 Up as PNG defines them, computed from the raw image: Up reads the row above also across a
 * band boundary, zeros above row 0).  Every band is deflated by one wavefront with the rule of dbm_chunk_encode, framed as a segment:
 * no zlib header and no Adler-32; one block with the fixed Huffman code, BFINAL 0, followed by an empty stored block (bits 000, padding
 * to a byte, 00 00 FF FF) -- or, for the image's last band, BFINAL 1 and padding.  78 01 + the segments in order + the big-endian
 * Adler-32 of all bands' bytes is one valid zlib stream.  out_host (HOST, out_capacity bytes) receives the segments one behind the
 * other, each at the next even offset from 0; sizes_host (HOST) their n_bands sizes, adlers_host (HOST) the Adler-32 of each band's
 * bytes.  out_capacity must cover the worst case: n_bands times n + n / 8 + 16 rounded up to even, n = min(band_rows, H) (W channels
 * + 1).  The call allocates its workspace (per band: the filtered band rounded up to 16, the slot of the worst case, 32 bytes of
 * bookkeeping; plus the packed segments), frees it on every path, synchronises the context's stream and writes no caller-visible
 * device memory; the caller bounds the workspace by batching.
 * Status 12: a band's segment did not fit its slot (the guard of the device loop; it cannot occur with the slot above).
 * Refused (status 1, nothing launched): NULL pointers, an empty image or H * W >= 2^31, channels not 1, 3 or 4, filter outside 0..2,
 * band_rows < 1, a band of 2^31 bytes or more, a band range outside the image, 2^31 workgroups or more, out_capacity below the worst
 * case.  n_bands = 0 succeeds.
 * dbm_png_encode_host (deepbedmap.py:758-775): the same bytes from a HOST image on `nthreads` host threads -- the device encoder's own
 * loop and the same filter text run with one lane.  No GPU, no context. */
int dbm_grid_relief(dbm_ctx* ctx, const float* plane_dev, long H, long W, const double* edges_host, const uint8_t* colors_host, int n_slices,
                    int channels, int shade, double sin_a, double cos_a, double aspect, double mean, double sigma, double k, uint8_t* out_dev);
int dbm_grid_shade_stats(dbm_ctx* ctx, const float* plane_dev, long H, long W, double sin_a, double cos_a, double aspect, double* out_host);
int dbm_png_encode(dbm_ctx* ctx, const uint8_t* image_dev, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                   void* out_host, size_t out_capacity, size_t* sizes_host, uint32_t* adlers_host);
int dbm_png_encode_host(const void* image, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands, void* out,
                        size_t out_capacity, size_t* sizes, uint32_t* adlers, int nthreads);

/* ---- the 3-D perspective view of the DEM (deepbedmap.py:258-295, `plot_3d_view`: `fig.grdview(..., surftype="sim", plane=zmin,
 * zscale=0.01, perspective=[202.5, 60])`).  A hidden-surface render of the height field under an orthographic view; the frame, the
 * view's angles and the product stay with the host shim deepbedmap_amd/perspective.py.  The rule is this project's own -- GMT's pixels
 * are not claimed -- and is stated operation by operation in DESIGN.md 6o and at the head of csrc/perspective.hip ----
 * dbm_grid_minmax (deepbedmap.py:258-295: the vertical range the frame is made from) returns out_host[3] = {count of finite samples,
 * min, max} of the float32 plane plane_dev (H, W), a DEVICE pointer; min and max are order-free and therefore exact; NaN, NaN if the
 * count is 0.  The call allocates its workspace, frees it on every path and synchronises.  Refused (status 1): NULL pointers, an empty
 * plane or H * W >= 2^31.
 * dbm_grid_perspective (deepbedmap.py:258-295) renders the plane plane_dev (H, W; rows north-up; node (r, c) at east c, north -r, height
 * h = (z - level) zfac) draped with drape_dev, uint8 (H, W, drape_channels) at the nodes (what dbm_grid_relief wrote for the plane; a
 * fourth channel is not read), into out_dev, uint8 (Ho, Wo, 4), and, unless NULL, the ids of the visible triangles into hits_dev,
 * int32 (Ho, Wo): 2 (r (W - 1) + c) + t for triangle t of cell (r, c), -2 a wall of the facade, -1 none.  plane, drape, out and hits
 * are DEVICE pointers.  view_host (HOST, nine doubles): sin A, cos A, sin E, tan E, level, zfac, sx0, sy0, step -- the caller computes
 * the functions of the azimuth A (clockwise from north, where the viewer stands) and of the elevation E once; pixel (i, j) looks along
 * the ray through screen point sx = sx0 + (j + 0.5) step, sy = sy0 - (i + 0.5) step.  facade_rgba (HOST, four bytes, or NULL: no
 * facade): the colour of the vertical walls between height 0 and the boundary profile on the four outer edges; background_rgba
 * (HOST, four bytes): the colour of a pixel that sees nothing.  Every operation of the pixel rule is one IEEE float64 operation,
 * never an FMA; the image does not depend on the traversal (blocks of 8 x 8 and 64 x 64 cells are skipped by their maxima; the walk
 * stops behind the visible hit).  H < 2 or W < 2 renders the background.  The call allocates its workspace (4 bytes per 8 x 8 block,
 * 12 per 64 x 64 block), frees it on every path and synchronises.
 * Refused (status 1, nothing launched): NULL pointers (but facade_rgba and hits_dev), drape_channels not 3 or 4, an empty plane or
 * image, H * W, Wo * Ho or 2 (H - 1) (W - 1) >= 2^31, a view value that is not finite, sin A^2 + cos A^2 off 1 by more than 1e-6,
 * sin E, tan E, zfac or step <= 0.
 * dbm_grid_perspective_host (deepbedmap.py:258-295): the same bytes from HOST arrays on `nthreads` host threads -- the kernel's own
 * cell, wall and colour functions under a PLAIN traversal: every cell the ray's ground line meets, no blocks, no early stop.  No GPU,
 * no context; the same refusals. */
int dbm_grid_minmax(dbm_ctx* ctx, const float* plane_dev, long H, long W, double* out_host);
int dbm_grid_perspective(dbm_ctx* ctx, const float* plane_dev, long H, long W, const uint8_t* drape_dev, int drape_channels, const double* view_host,
                         long Wo, long Ho, const uint8_t* facade_rgba, const uint8_t* background_rgba, uint8_t* out_dev, int32_t* hits_dev);
int dbm_grid_perspective_host(const float* plane, long H, long W, const uint8_t* drape, int drape_channels, const double* view, long Wo, long Ho,
                              const uint8_t* facade_rgba, const uint8_t* background_rgba, uint8_t* out, int32_t* hits, int nthreads);

/* One minibatch of `trainer` (srgan_train.py:1286-1309) as ONE call: train_eval_discriminator (:1084-1166) with its
 * optimizer update, then train_eval_generator (:1170-1263) with its update; both optimizers must have been set up
 * (dbm_adam_setup).  Numerically the two step calls + two dbm_adam_update calls, bit for bit; scheduled as a whole: the
 * generator's backward pass -- independent of everything the D-step computes, since the adversarial term is detached
 * (:1228-1229) -- runs on a library stream underneath the discriminator's backward passes.  metrics_dev (device, >= 8
 * floats) receives [d_loss, d_accu, g_loss, psnr, ssim].  With a communicator on the context (dbm_comm_init /
 * dbm_comm_set_hook) the call is one data-parallel iteration: both models' gradient buckets are summed over ranks inside
 * it (on library stream chain[0], underneath the generator's backward pass) and both updates take 1 / world -- the same
 * collectives in the same order as the two step calls.  Refused with sync_batch_stats (use the two step calls).
 * flags: 0 or DBM_ONE_GEN_FORWARD.  All five metrics are complete when the call's work is. */
int dbm_train_iteration(dbm_model* g, dbm_model* d, int N, int H, int W, const float* X, const float* W1, const float* W2,
                        const float* W3, const float* Y, const float weights[4], int ssim_window, int flags,
                        float* metrics_dev);

/* ---- op-level entry points (used by the parity tests; same kernels the models run) ---- */
/* L.Convolution2D forward on the MFMA implicit-GEMM kernel. x (N,C,H,W) w (O,C,k,k) b (O) or NULL -> y; all DEVICE. */
int dbm_op_conv2d(dbm_ctx* ctx, const float* x, const float* w, const float* b, float* y, int N, int C, int H, int W,
                  int O, int k, int stride, int pad, int upsample2, int lrelu);
/* data gradient (gx, may be NULL) and weight/bias gradient (gw, gb accumulated; may be NULL) of the same layer */
int dbm_op_conv2d_backward(dbm_ctx* ctx, const float* x, const float* w, const float* gy, float* gx, float* gw,
                           float* gb, int N, int C, int H, int W, int O, int k, int stride, int pad, int upsample2);
/* One forward or data-gradient launch of the same layer exactly as the models make it (fwd_desc / dgrad_desc + run_dgrad with every
 * epilogue field, strided operands); all DEVICE pointers.  With acc = the convolution sum for output channel c:
 *   v = (acc * ch_scale[c] + bias[c]) * s1 + (c < r1_nch ? r1s * r1 : 0);  if (r2) v = s2 * v + r2;  if (accumulate) v += y;
 *   if (act) v = lrelu_0.2(v);  if (mask && c >= mask_c0) v *= (mask >= 0 ? 1 : 0.2)
 * r1, r2, mask are addressed like y (same channel plane, same position) with their own image strides.  The layer is (O, C, k, k),
 * stride, pad, on an H x W input plane (ups = 1: x holds H x W, the layer sees the nearest x2 resize).
 *   dgrad = 0: x (N, >= C, H, W) with image stride xsn -> y (N, >= O, OH, OW) with image stride ysn; bias (O) or NULL; yt (N * OH * OW, 64) or
 *              NULL is handed to the launch only where the model would (conv_tile_writes_yt).
 *   dgrad = 1: x = dy (N, >= 32 * ceil(O / 32) channel planes, OH, OW; planes >= O hold zeros) -> y = gx (N, >= C, H, W); ups, bias,
 *              ch_scale, yt must be 0 / NULL.  A stride-2 layer is the four-phase launch, or one launch per phase on a plane one pixel wide.
 * report (HOST, may be NULL, 41 ints): report[0] = launches made (1, or up to 4), then ten ints per launch:
 *   family (0 igemm_conv_kernel, 1 igemm_pm_kernel, 2 conv_tile_kernel), conv_tile cfg (1..6, else 0), wavefronts per workgroup,
 *   NPB (0 streaming, 6 register-resident, -1 tap-skip, -2 bf16, -4 two tiles), ROW, ksplit, nosplit, nphase, two output tiles per
 *   wavefront, yt written. */
typedef struct dbm_conv_launch {
  int dgrad;
  int N, C, H, W, O, k, stride, pad, ups;
  const float* w;      /* OIHW (O, C, k, k), contiguous */
  const float* bias;
  const float* x; int64_t xsn;
  float* y; int64_t ysn;
  int act; float s1;
  const float* r1; int64_t r1sn; int r1_nch; float r1s;
  const float* r2; int64_t r2sn; float s2;
  int accumulate;
  const float* mask; int64_t masksn; int mask_c0;
  const float* ch_scale;
  float* yt;
} dbm_conv_launch;
int dbm_op_conv2d_launch(dbm_ctx* ctx, const dbm_conv_launch* args, int* report);
/* L weight gradients as ONE batch, the training step's form: gW (O, C, k, k) += scale * sum dy * x, gb (O, or NULL) += scale * sum dy, for
 * x (N, >= C, H, W; C % 4 == 0, C >= 32) with image stride xsn (ups = 1: the layer sees its nearest x2 resize) and dy (N, >= O, OH, OW) with image stride dysn.
 * Two descriptors may name the same gW / gb (the real and the fake graph).  cleared_target = 1: the caller guarantees every gW / gb is
 * zero and receives nothing else.  dbm_set_deterministic selects the folding; a call with the descriptors of the previous call reuses
 * its batch (a mode switch re-plans it).  cat_out / S_out (HOST, L ints each, may be NULL): per descriptor the kernel category (-1
 * wgrad_s2tiny_kernel; 0 1x1, 1 3x3 and 2 4x4 workgroup form; 3 3x3 wave LDS-DMA; 4 / 5 3x3 / 4x4 row-band LDS-DMA; 6 / 7 / 8 direct
 * form 3x3 / 3x3 on a resized input / 4x4 stride 2; 9 1x1 on large planes) and its number of K slices. */
typedef struct dbm_wgrad_desc {
  const float* x; int64_t xsn;
  const float* dy; int64_t dysn;
  int N, C, H, W, O, k, stride, pad, ups;
  float scale;
  float* gW;
  float* gb;
} dbm_wgrad_desc;
int dbm_op_conv2d_wgrad_batch(dbm_ctx* ctx, const dbm_wgrad_desc* descs, int L, int cleared_target, int* cat_out, int* S_out);
/* The persistent trunk kernels (trunk_fused.hip, trunk_fused_bwd.hip) through the models' own path: the weight streams are packed from
 * plain OIHW tensors (launch_pack_trunk_fused / launch_pack_trunk_fused_bwd), the launch loop is Generator::forward's / backward's, chunk
 * by chunk between persist_begin / persist_end, with the context's error words.  All pointers are HOST pointers: every buffer goes up
 * whole and comes back whole, so what a launch did not write comes back as the caller left it.  Planes are 9 x 9; a concat buffer is
 * (N, 192, 81): channels 0..63 the dense block's input, 64..191 conv_layer1..4's outputs.
 *   nrdb: dense blocks, a multiple of 3 with nrdb + 1 <= 64 (TRUNK_FUSED_MAXCAT; anything else is refused, nothing launched)
 *   w, b: tables of nrdb * 5 pointers, dense block j's conv_layer(k + 1) at [5 j + k]: (32, 64 + 32 k, 3, 3) / (32), conv_layer5 (64, 192, 3, 3) / (64)
 *   imgs_per_launch: 1 .. the context's images per persistent launch (min(64, CUs / 3)); launch c covers images [c * imgs_per_launch, ...)
 *   only_launch: >= 0 runs that chunk's launch(es) alone (the other images are not touched), -1 all
 *   epoch0: the first launch's epoch, the following launches count up from it (the kernels use its low 20 bits); negative: the context's
 *           counter goes on.  The two ops share ONE inbox of trunk_fused_inbox_bytes(64) bytes (zeroed once per context) and that counter,
 *           as a generator's workspace does.
 *   agent_stores: 1 = exchange stores at agent scope only (what the kernels do after a time-out), 0 = same-XCD stores may stay in the L2
 * report (HOST, report_cap ints, may be NULL): report[0] = launches made, then per launch {form, workgroups}: form 0 = 27-position tiles,
 *   1 = the same with a helper workgroup per image, 2 = 32-position tiles, 3 = the data-gradient chain.  The launcher takes the helper
 *   form only while four workgroups per image fit the device; the report says what ran.
 * A call returns status 7 when a bounded spin ran out (the error word was raised); the op lowers the word again and touches no model.
 *
 * dbm_op_trunk_forward (srgan_train.py:333-360, :393-404, :546): cat[0][:, 0:64] is the trunk input.  keep = 1: cat is a table of nrdb + 1
 *   buffers, every layer's output is stored (cat[j][:, 64:192], cat[j + 1][:, 0:64]); keep = 0: cat[0] only, the trunk's output goes to
 *   out[:, 0:64] (N, 192, 81).  tile: 27 or 32; helper: 1 asks for the helper form (tile 27 only). */
typedef struct dbm_trunk_forward {
  int nrdb, N;
  float rs;
  int imgs_per_launch, only_launch, epoch0;
  int keep, tile, helper, agent_stores;
  const float* const* w;
  const float* const* b;
  float* const* cat;
  float* out;
} dbm_trunk_forward;
int dbm_op_trunk_forward(dbm_ctx* ctx, const dbm_trunk_forward* args, int* report, int report_cap);
/* dbm_op_trunk_backward: the data-gradient chain, nlaunch launches (j0[i], j1[i]) from the top of the trunk down, each over whole RRDBs
 *   (multiples of 3, j0 < j1 <= nrdb), each starting where the one before ended (j1[i] = j0[i - 1]).  The first launch's incoming
 *   gradient is gin (N images of gin_sn floats, 64 * 81 or 192 * 81, channels 0..63 are read); a later one reads dA[j1][:, 0:64].  cat and
 *   dA are tables of nrdb buffers (N, 192, 81): cat[j] supplies the LeakyReLU masks (value >= 0: derivative 1), dA[j] receives block j's
 *   concat gradient -- channels 64..191 the gradients of conv_layer1..4's outputs in front of their LeakyReLU, channels 0..63 the gradient of
 *   the block's input.  g_a3 (N, 64, 81) is added at block 0, whose channels 0..63 then pass cat[0]'s mask. */
typedef struct dbm_trunk_backward {
  int nrdb, N;
  float rs;
  int imgs_per_launch, only_launch, epoch0;
  int agent_stores;
  int nlaunch;
  const int* j0;
  const int* j1;
  const float* const* w;
  const float* gin; int64_t gin_sn;
  const float* const* cat;
  const float* g_a3;
  float* const* dA;
} dbm_trunk_backward;
int dbm_op_trunk_backward(dbm_ctx* ctx, const dbm_trunk_backward* args, int* report, int report_cap);
/* the same L.Convolution2D (3x3, stride 1, pad 1: the RRDB trunk's layers, srgan_train.py:292-331) on the channels-last
 * bf16 kernel of the area sweep (conv_cl16.hip): x is rounded to bf16, fp32 accumulation, y = [lrelu](s1 * (conv + b) + r1)
 * with r1 (N,64,H,W) or NULL; C % 32 == 0, O = 32 or 64 */
int dbm_op_conv2d_cl16(dbm_ctx* ctx, const float* x, const float* w, const float* b, const float* r1, float s1, float* y, int N,
                       int C, int H, int W, int O, int lrelu);
/* ... and in the sweep's split-bf16 arithmetic (three bf16 MFMAs per product: operands carry 16 significand bits) for the
 * layers on the signal path -- post_upsample_conv_layer_1/2 behind F.resize_images (srgan_train.py:553-568; ups = 1: x is the
 * (H/2, W/2) plane) and the deformable layers' offset convolutions (:506-523; planar = 1: channel-plane output):
 * x (N,64,H>>ups,W>>ups) -> y (N,O,H,W), O <= 64 */
int dbm_op_conv2d_cl16x3(dbm_ctx* ctx, const float* x, const float* w, const float* b, float* y, int N, int H, int W, int O, int ups,
                         int lrelu, int planar);
/* L.DeformableConvolution2D sampler + GEMM (stride 1, pad 1, 3x3): off (N,18,H,W) */
int dbm_op_deform_conv2d(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* b, float* y,
                         int N, int C, int H, int W, int O);
/* the two other forms of the forward pass the generator uses, 64 input channels: form 1 = the few-output-channel layer
 * (O <= 16; srgan_train.py:574, the DEM itself) with the multiplication BEFORE the sampler -- nine premultiplied tap planes,
 * scalar gathers --, form 2 = the 64 -> 64 layer (:572) in the sweep's split-bf16 arithmetic (+ LeakyReLU 0.2 if lrelu); forms 3 and 4
 * name form 2's two kernels explicitly -- 3: the sampler reads an LDS window of the input (what the sweep's full-resolution planes take),
 * 4: it gathers every corner from memory (small planes); same arithmetic, same bits.  Form 3 is refused (DBM_CHECK naming the limits)
 * on planes past its kernel's limits (H <= 32765, W <= 65533, H * W < 2^24); form 2 takes form 4's kernel there */
int dbm_op_deform_conv2d_form(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* b, float* y, int N, int H,
                              int W, int O, int form, int lrelu);
int dbm_op_deform_conv2d_backward(dbm_ctx* ctx, const float* x, const float* off, const float* w, const float* gy,
                                  float* gx, float* goff, float* gw, float* gb, int N, int C, int H, int W, int O);
/* One deformable forward (64 input channels, 3x3, pad 1) launched exactly as the generator launches it (srgan_train.py:572-574): the
 * offsets off (N, >= 18, H, W) at their own image stride offsn in floats (the generator's live in a 32-channel buffer), LeakyReLU 0.2
 * if act, and the optional outputs, each handed to the launcher as given (NULL stays NULL): y (N, O, H, W); yt (N * H * W, 64), the
 * same values channels-last (O = 64; y may then be NULL); colout (N, 576, H, W), the sample matrix, row c * 9 + t (O = 64, fp32); z
 * (N, O, 9, H, W), the premultiplied planes sum_c w[o, c, t] x[c] (O <= 16).  form: 0 the layer's own choice, on the packed temporary
 * layer (a layer that premultiplies gets a scratch z where z is NULL, as the generator's workspace has one); 1 premultiplied (O <= 16);
 * 2 / 3 / 4 split-bf16, the launcher's choice / its LDS-window kernel / its gathering kernel (O = 64); 5 gather, then multiply (O <= 16,
 * z == NULL); 6 the unfused path: the sampler writes the sample matrix (into colout where given), then a GEMV (O = 1) or the implicit
 * GEMM (O % 32 == 0).  Combinations the launchers do not support are refused.  report (HOST, one int, may be NULL): the path taken --
 * 1 launch_deform_conv_fused 64 -> 64 (LDS-window kernel without colout on planes within its limit, else the gathering kernel; the
 * profiler's tag tells: deform64w_... / deform64_...[_keep]), 2 premultiplied, 3 gather-then-multiply, 4 launch_deform_conv64_x3
 * (deform64x3w_... / deform64x3_...), 5 sampler + GEMV, 6 sampler + implicit GEMM. */
typedef struct dbm_deform_launch {
  int form;
  int N, H, W, O;
  int act;
  const float* x;      /* (N, 64, H, W) */
  const float* off; int64_t offsn;
  const float* w;      /* OIHW (O, 64, 3, 3) */
  const float* bias;   /* O, or NULL */
  float* y;
  float* yt;
  float* colout;
  float* z;
} dbm_deform_launch;
int dbm_op_deform_forward_launch(dbm_ctx* ctx, const dbm_deform_launch* args, int* report);
/* L.BatchNormalization (training mode, eps 1e-5, decay 0.9) + F.leaky_relu(0.2) as the discriminator runs them (srgan_train.py:636-644,
 * 664-689): z (N,C,plane) -> y, per-channel mean / inv_std (C) overwritten; avg_mean / avg_var (C) updated in place with the unbiased
 * correction m / max(m - 1, 1), m = N * plane.  The kernel form is the model's own launch choice for (N, C, plane); *form_out (HOST, may
 * be NULL) receives it: 0 reg<2>, 1 reg<6>, 2 flat<1>, 3 flat<4>, 4 the 1024-thread general kernel, 5 the 256-thread general kernel.
 * sync = 1: the sync_batch_stats kernels (local statistics, then apply) at world = 1 without an all-reduce; *form_out = -1. */
int dbm_op_batchnorm_train(dbm_ctx* ctx, const float* z, const float* gamma, const float* beta, float* avg_mean, float* avg_var, float* y,
                           float* mean, float* inv_std, int N, int C, int plane, int sync, int* form_out);
/* ... and their backward pass: gh = d loss / d y -> gz (overwritten); ggamma / gbeta (C) are ACCUMULATED (atomicAdd).  mean / inv_std:
 * what the forward pass wrote. */
int dbm_op_batchnorm_train_backward(dbm_ctx* ctx, const float* z, const float* gh, const float* gamma, const float* beta, const float* mean,
                                    const float* inv_std, float* gz, float* ggamma, float* gbeta, int N, int C, int plane, int sync,
                                    int* form_out);
/* linear_1 (512 -> 100) -> LeakyReLU -> linear_2 (100 -> 1), the discriminator's head (srgan_train.py:646-647, 693-696): x (N,512),
 * W1 (100,512), b1 (100), W2 (1,100), b2 (1) -> l1 (N,100) after the LeakyReLU, logits (N) */
int dbm_op_disc_head(dbm_ctx* ctx, const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* l1,
                     float* logits, int N);
/* ... and its backward pass from glogits (N): gx (N,512) overwritten; gW1, gb1, gW2, gb2 ACCUMULATED.  The model's own sequence: one fused
 * launch while 4 * N * 100 bytes fit 48 KiB of LDS, else one launch per linear layer; *fused_out (HOST, may be NULL) = 1 / 0. */
int dbm_op_disc_head_backward(dbm_ctx* ctx, const float* x, const float* W1, const float* W2, const float* glogits, const float* l1, float* gx,
                              float* gW1, float* gb1, float* gW2, float* gb2, int N, int* fused_out);
/* DeepbedmapInputBlock (srgan_train.py:223-266) through the generator's own launch sequences: x (N,1,H,W), w1 (N,1,10H,10W),
 * w2 (N,2,2H,2W), w3 (N,1,H,W); wx / bx, ww1 / b1, ww2 / b2, ww3 / b3: the OIHW weights (32,1,3,3), (32,1,30,30), (32,2,6,6), (32,1,3,3)
 * and biases (32) of conv_on_X, _W1, _W2, _W3; all DEVICE -> y (N, 128, plane = (H-2)(W-2)) with image stride ysn >= 128 * plane.  yt (N * plane, 128) or NULL: the concat
 * channels-last INSTEAD of y (y is then left alone), form 2 only.  form: -1 the model's own choice for these pointers and this shape,
 * 0 layer-wise (im2col + GEMM for the wide branches, the few-channel kernel for the 3x3 ones), 1 the fused kernel of the 11 x 11
 * training tile (w1 and w2 16-byte aligned), 2 the rows kernel (H >= 3, W >= 66).  A form that the shape or the alignment does not allow
 * is refused (DBM_CHECK naming the condition), and so is yt outside form 2.  *form_out (HOST, may be NULL): the form that ran. */
int dbm_op_input_block(dbm_ctx* ctx, const float* x, const float* w1, const float* w2, const float* w3, const float* wx, const float* bx,
                       const float* ww1, const float* b1, const float* ww2, const float* b2, const float* ww3, const float* b3, float* y,
                       int64_t ysn, float* yt, int N, int H, int W, int form, int* form_out);
/* ... and its weight gradients from g (N, >= 128, plane) with image stride gsn, as Generator::backward runs them behind a fused forward:
 * the wide branches' im2col images rebuilt from w1 / w2, the two branches as 1x1 layers of 900 / 72 channels in ONE batch (folding by
 * dbm_set_deterministic), the 3x3 branches through the few-channel kernel without scratch; on the context's side stream.  The four
 * gradient pairs (gwx / gbx, gw1 / gb1, gw2 / gb2, gw3 / gb3, shapes as the weights above) are ACCUMULATED.  cat_out / S_out (HOST,
 * 2 ints each, may be NULL): category and K slices of the W1 and the W2 branch, as dbm_op_conv2d_wgrad_batch reports them. */
int dbm_op_input_block_backward(dbm_ctx* ctx, const float* x, const float* w1, const float* w2, const float* w3, const float* g, int64_t gsn,
                                float* gwx, float* gbx, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3, int N, int H,
                                int W, int* cat_out, int* S_out);
/* Weight gradient of a few-input-channel convolution (the input block's branches, the discriminator's conv_layer0) through
 * launch_smallcin_conv_wgrad: x (N,C,H,W), gy (N,O,OH,OW) -> gw (O,C,k,k) and gb (O, or NULL) ACCUMULATED.  with_scratch = 1: the launch
 * is handed a scratch buffer as the discriminator hands it one.  *form_out (HOST, may be NULL): 0 one workgroup per gradient element,
 * 1 partial sums per position slice + fold (with scratch, one channel, 3x3, stride 1, pad 1, O % 8 == 0, N * OH * OW >= 16384). */
int dbm_op_smallcin_wgrad(dbm_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int N, int C, int H, int W, int O, int k,
                          int stride, int pad, int with_scratch, int* form_out);
/* Backward of F.resize_images x2 (nearest; srgan_train.py:556-566) with the LeakyReLU(0.2) derivative of the layer below: g (nc, 2H, 2W)
 * -> out (nc, H, W) = (g00 + g01) + (g10 + g11), times 0.2 where mask (nc, H, W, or NULL) < 0 (both zeros: derivative 1) */
int dbm_op_sumpool2(dbm_ctx* ctx, const float* g, const float* mask, float* out, int64_t nc, int H, int W);

/* ---- reading survey text tables: the `pandas.read_csv` + `dropna` of ascii_to_xyz (data_prep.py:298-305) ----
 * text: nbytes bytes of one file, host or (DBM_DEVICE_PTRS) device, a device pointer 16-byte aligned; offsets are 64-bit, files above
 * 4 GiB work.  The dialect: lines end at '\n', one '\r' before it is dropped, a last line without '\n' counts.  A line is
 * blank when it holds nothing but spaces and tabs (a tab is not blank space when it is the separator); blank lines are skipped, then the
 * first skip + 1 non-blank lines are discarded unparsed (`header=skip`: the line after the skipped ones is taken for the header, so with
 * skip = 1 and one header line the first data row is lost, as in the reference).  separator: ',' or '\t' (every occurrence separates),
 * or DBM_TEXT_SEP_WHITESPACE (maximal runs of spaces and tabs separate, leading and trailing runs are ignored).  Quotes are NOT
 * interpreted.  Field f of a line belongs to name f of nfields names; bit f of use_mask marks it used; the table's columns are the used
 * fields in file order.  Only used fields are looked at.  A used field, trimmed of spaces and tabs, is NaN if it is empty, equals one of
 * the n_na strings of na_values (NUL-terminated one after the other, each 1..DBM_TEXT_MAX_NA_BYTES bytes, compared byte for byte -- NOT
 * pandas' numeric comparison) or one of pandas' default NA strings (#N/A, #N/A N/A, #NA, -1.#IND, -1.#QNAN, -NaN, -nan, 1.#IND, 1.#QNAN,
 * <NA>, N/A, NA, NULL, NaN, None, n/a, nan, null); +-inf for [+-]?(inf|infinity) in any case; the correctly rounded double for
 * [+-]?(digits[.digits*] | .digits)([eE][+-]?digits)?; anything else is an error.  A field missing at the end of a short line is NaN; a
 * line with more than nfields fields is an error.  A row is kept unless a used field is NaN (+-inf is kept), in file order.
 * The device converts a number exactly when its significant digits (at most 19) give an integer w <= 2^53 and its decimal exponent e
 * has |e| <= 22: double(w) * 10^e or double(w) / 10^-e, one IEEE operation on exact operands.  Any other number is NOT guessed: the row
 * is kept, its other fields converted, and (byte offset of its line, its row in table_out) appended to the repair list, in file order;
 * the caller converts that line (strtod, Python float) and patches the row.
 *
 * dbm_text_count_lines: counts_out (HOST, 2) = {lines, non-blank lines}; max(0, non-blank lines - skip - 1) bounds the rows of any
 * parse of this text.  Synchronises.
 * dbm_text_parse: table_out (table_capacity rows of popcount(use_mask) doubles; host or, with DBM_DEVICE_PTRS, device), repair_out
 * (HOST, repair_capacity pairs of int64; may be NULL with capacity 0), result_out (HOST, 4) = {rows kept, repair pairs, byte offset of
 * the FIRST line in file order that holds an error or -1, candidate lines}.  With an error nothing is written to table_out and rows
 * kept = repair pairs = 0 (status 0: the caller names the line).  The call reads counts back twice, so it synchronises even with
 * DBM_DEVICE_PTRS; its scratch (8 popcount + 9 bytes per candidate line) is freed on every path.  Kept rows are compacted with flags
 * and an exclusive scan, no atomic append: the same bytes from call to call.  Status 1 (refused, nothing written): a separator other
 * than the three, skip < 0, nfields outside 1..DBM_TEXT_MAX_FIELDS, use_mask empty or with a bit at or above nfields, n_na outside
 * 0..DBM_TEXT_MAX_NA or a string outside 1..DBM_TEXT_MAX_NA_BYTES bytes, a misaligned device pointer, NULL pointers, table_capacity <
 * rows kept, repair_capacity < repair pairs.
 *
 * dbm_text_columns: the steps of ascii_to_xyz behind the read (data_prep.py:298-305 the table, :307-320 `df.eval("A-B")`, `drop`, the
 * columns sorted by name).  in_dev (n, ncol_in) and out_dev (n, ncol_out) are float64 DEVICE tables that do not overlap; column c of
 * out is column a[c] of in (op[c] = 0), a[c] + b[c] (op[c] = 1) or a[c] - b[c] (op[c] = 2): one IEEE operation, no contraction.  a, op,
 * b: HOST arrays of ncol_out ints (the expression is parsed by the caller).  Asynchronous.  Status 1: ncol_out outside
 * 1..DBM_TEXT_MAX_COLUMNS, ncol_in < 1, an index outside the input's columns, an op outside 0..2, NULL pointers with n > 0. */
int dbm_text_count_lines(dbm_ctx* ctx, const void* text, size_t nbytes, int separator, int64_t* counts_out, int flags);
int dbm_text_parse(dbm_ctx* ctx, const void* text, size_t nbytes, int separator, int skip, int nfields, uint64_t use_mask,
                   const char* na_values, int n_na, double* table_out, size_t table_capacity, int64_t* repair_out, size_t repair_capacity,
                   int64_t* result_out, int flags);
int dbm_text_columns(dbm_ctx* ctx, const double* in_dev, size_t n, int ncol_in, double* out_dev, int ncol_out, const int* a, const int* op,
                     const int* b);

#ifdef __cplusplus
}
#endif
#endif
