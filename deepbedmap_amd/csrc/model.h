// Model objects behind the C ABI: parameter tables in chainer save_npz key order, packed-weight
// caches for the MFMA kernels, activation workspaces, forward/backward orchestration.
#pragma once
#include "dbm_internal.h"
#include "kernels.h"
#include "../../include/dbm.h"

struct DevBuf {
  float* p = nullptr;
  size_t n = 0;
  void ensure(size_t count);  // room for `count` floats; only grows, and a fresh allocation is zeroed
  // the same for `count` elements of T (bytes: T = char), rounded up to whole floats: callers that think in doubles or bytes
  // state their size in their own unit
  template <class T> T* as(size_t count) {
    ensure((count * sizeof(T) + sizeof(float) - 1) / sizeof(float));
    return reinterpret_cast<T*>(p);
  }
  void release();
};

// A temporary of one call: released when the scope ends, also when a DBM_CHECK throws on the way.
struct ScopedBuf : DevBuf {
  ScopedBuf() = default;
  ScopedBuf(const ScopedBuf&) = delete;
  ScopedBuf& operator=(const ScopedBuf&) = delete;
  ~ScopedBuf() { release(); }
};

struct dbm_ctx {
  explicit dbm_ctx(int hip_device) : device(hip_device) {}
  dbm_ctx(const dbm_ctx&) = delete;
  ~dbm_ctx();  // (model.hip) frees and destroys everything declared below; dbm_init fills it in, dbm_shutdown drains the streams first
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  hipStream_t side = nullptr;        // library-owned side stream: independent work overlapping the main chain
  hipEvent_t ev_fork[8] = {};        // main -> side dependencies
  hipEvent_t ev_join = nullptr;      // side -> main
  hipStream_t chain[2] = {};         // library-owned streams: second image range of the 9x9 stage / fake-batch D backward;
                                     // main stream of a prefetched generator forward (never more than four streams busy)
  void fork(hipStream_t from, hipStream_t to, int k);  // `to` waits for everything enqueued on `from` so far
  void fork_to_side(int k);          // side waits for everything enqueued on `stream` so far
  void join_side();                  // `stream` waits for everything enqueued on `side` so far
  std::string err;
  // sync_batch_stats (dbm_set_sync_batch_stats): > 1 = BatchNorm / RaGAN statistics are summed over `sync_world` ranks by
  // the caller's hook, which must enqueue the collective on `stream`
  int sync_world = 1;
  void (*sync_fn)(void* user, float* dev, int n) = nullptr;
  void* sync_user = nullptr;
  bool sync_stats() const { return sync_world > 1 && (sync_fn != nullptr || nccl_comm != nullptr); }
  void allreduce(float* dev, int n);  // statistics collective on `stream`: the hook, or the native communicator
  DevBuf sync_buf;            // 3 x 512 floats of per-channel sums + 4 for the loss
  // ---- gradient exchange of a data-parallel run (comm.hip): native RCCL communicator, or a caller hook ----
  void* nccl_comm = nullptr;  // ncclComm_t (dbm_comm_init)
  int comm_rank = 0, comm_world = 1;
  void (*comm_hook)(void* user, float* dev, size_t n, void* hip_stream) = nullptr;  // dbm_comm_set_hook
  void* comm_user = nullptr;
  bool comm_in_step = false;  // set by the fused steps: the backward passes hand finished buckets to comm_bucket
  hipStream_t comm_stream = nullptr;  // stream the collectives are enqueued on (null: chain[1]; dbm_train_iteration: chain[0])
  bool comm_defer = false;    // comm_bucket only records the producers' event; the all-reduce goes out with comm_flush()
  struct PendingBucket { float* p[2]; size_t n[2]; int nranges; hipEvent_t ev; };
  std::vector<PendingBucket> comm_pending;
  std::vector<hipEvent_t> comm_ev_pool;  // one event per bucket of a pass (reused from pass to pass)
  size_t comm_ev_used = 0;
  void comm_flush();
  hipEvent_t ev_comm = nullptr, ev_comm_done = nullptr;
  hipEvent_t ev_timer[2] = {nullptr, nullptr};  // dbm_timer
  hipEvent_t ev_iter[4] = {nullptr, nullptr, nullptr, nullptr};   // dbm_train_iteration: loss scratch cleared / generator backward done /
                                                                // G grads cleared + its data-gradient images / D's data-gradient images
  // The persistent trunk kernels need every workgroup of a launch resident at once: two of them on different streams, each
  // holding part of the chip, would wait for each other's compute units until their spin limits.  Every persistent launch
  // therefore waits for the previous one (whatever its stream) and leaves its own completion here.
  hipEvent_t ev_persist = nullptr;
  bool persist_pending = false;
  void persist_begin(hipStream_t s);
  void persist_end(hipStream_t s);
  size_t comm_bytes = 0, comm_calls = 0;  // statistics (dbm_comm_stats)
  // DBM_COMM_FORCE_WORLD1=1 (testing / measuring the data-parallel schedule on ONE GPU): a one-rank communicator counts as
  // active -- every bucket really goes through ncclAllReduce (a sum over one rank), the persistent launches keep to 192
  // workgroups, the optimizers wait for the exchange events
  static bool comm_force_world1() {
    static const bool f = getenv("DBM_COMM_FORCE_WORLD1") && atoi(getenv("DBM_COMM_FORCE_WORLD1")) != 0;
    return f;
  }
  bool comm_active() const {
    return (comm_world > 1 || (comm_force_world1() && comm_world == 1 && nccl_comm != nullptr)) && (nccl_comm != nullptr || comm_hook != nullptr);
  }
  void comm_init(int rank, int world, const void* id128);
  void comm_set_hook(int rank, int world, void (*fn)(void*, float*, size_t, void*), void* user);
  void comm_destroy();
  void comm_allreduce(float* const* p, const size_t* n, int nranges, hipStream_t on);
  void comm_broadcast(float* p, size_t n, int root, hipStream_t on);
  void comm_bucket(float* const* p, const size_t* n, int nranges, hipStream_t producer);
  void comm_bucket(float* p, size_t n, hipStream_t producer) { comm_bucket(&p, &n, 1, producer); }
  void comm_join(hipStream_t consumer);
  int trunk_imgs = 64;        // images per launch of the persistent trunk kernels: min(64, CUs / 3) (one workgroup per CU)
  std::vector<struct dbm_model*> models;  // every model of this context (optimizer bookkeeping after a kernel timeout)
  long data_epoch = 0;        // bumped by every entry point that writes / frees caller-visible device memory (note_device_write)
  int* dev_err = nullptr;     // host-mapped word a persistent kernel raises when a bounded spin runs out (checked by every API call)
  int* dev_err_d = nullptr;   // its device address
  int* dev_err_flag = nullptr;  // the same flag in device memory, STICKY until the host handles it (the optimizer launches and
                                // BatchNorm's running-average writes are no-ops while it is set)
  long timeout_events = 0;      // persistent-kernel timeouts handled so far (dbm_timeout_info)
  int timeout_skipped[2] = {0, 0};  // optimizer updates (discriminator, generator) that were no-ops in the last event
  float* zeros = nullptr;     // 256 B of zeros (igemm out-of-image taps)
  float* ssim_win[2] = {nullptr, nullptr};  // 9-tap 1-D windows: gaussian(1.5), uniform
  DevBuf loss_tmp;            // scratch for the loss entry points
  DevBuf stage[8];            // host<->device staging for the non-DEVICE_PTRS entry points
  DevBuf track_tmp;           // dbm_grid_track: the workgroups' error moments and the folded statistics (doubles)
  DevBuf tile_tmp;            // dbm_grid_filled_windows: the row pass's byte plane
  DevBuf resample_tmp;        // dbm_grid_rescale: min / max, Gaussian weights and the float64 planes (doubles)
  DevBuf points_tmp;          // dbm_points_region: the workgroups' boxes; dbm_points_blockmedian: block indices, histogram, scan, lists
  long long poly_stats[6] = {};  // list sizes of the last successful dbm_grid_polygon_mask (dbm_grid_polygon_stats)
  long long overlay_stats[4] = {};  // the same of the last successful dbm_image_overlay (dbm_image_overlay_stats)
  // What the op-level entry points (api_ops.hip) keep from call to call, made on first use on this context's device.
  struct OpState {
    // One inbox and one launch counter for both trunk ops: successive calls meet each other's granules, as the passes of a generator's
    // workspace do.  The counter starts in the middle of the 20-bit range, so that a context crosses the wrap only where a caller
    // asks for it (epoch0).
    unsigned long long* trunk_inbox = nullptr;
    int trunk_epoch = 0x80000;
    WgradBatch wgrad_batch;                    // dbm_op_conv2d_wgrad_batch: the batch of the previous call ...
    std::vector<dbm_wgrad_desc> wgrad_key;     // ... and the descriptors it was planned for
  } op;
};

void dbm_comm_unique_id_impl(void* out128);  // comm.hip: ncclGetUniqueId
// A persistent trunk kernel timed out: the layer-by-layer trunk path serves until iteration g_trunk_rearm_at (-1: for good);
// g_step_serial counts the training iterations entered (api.hip: dbm_step_entry).
// (These three and g_trunk_local_off (kernels.h) stay process-wide on purpose: a time-out on one context switches every context's trunk path.)
extern bool g_trunk_fused_off;
extern long g_step_serial, g_trunk_rearm_at;

struct Tensor {
  std::string key;
  int ndim;
  int64_t shape[4];
  int kind;
  size_t off;  // float offset inside the param (kind 0) or persistent (kind 1) arena
  size_t n;
};

// one L.Convolution2D executed by the implicit-GEMM kernel
struct IgLayer {
  int wi = -1, bi = -1;  // tensor indices (bias may be -1)
  int O = 0, C = 0, K = 0, stride = 1, pad = 1;
  int Cview = 0, Kview = 0;  // the (C, K) the GEMM sees (deform_conv: C*9, 1)
  int CinP = 0, CoutP = 0;
  float* wf = nullptr;       // [T][CinP][CoutP]
  void* wf16 = nullptr;      // bf16 [T][CinP/16][2][CoutP][8]: a lane's eight K values of one MFMA are one 16-byte load
  bool want_cl16 = false;    // also a fragment-ordered bf16 image for the channels-last kernel (conv_cl16.hip): trunk layers
  void* wcl16 = nullptr;     // bf16 [chunk][tap][k half][mtile][lane][8]
  bool want_x3 = false;      // ... and a split-bf16 (hi | lo) image for conv_cl16x3_kernel: the sweep's upsampling / offset convs
  void* wx3 = nullptr;       // bf16 [chunk][tap][mtile][hi | lo][lane][8]
  bool want_dx3 = false;     // the 64 -> 64 deformable layer: split-bf16 image for deform_conv64_x3_kernel (launch_pack_deform_x3)
  void* wdx3 = nullptr;
  int OP = 0, CP = 0;
  float* wb[4] = {nullptr, nullptr, nullptr, nullptr};  // dgrad packs [Tb][OP][CP]
  int Tb = 0;
  bool lazy = false;  // packed on demand only (dbm_model::ensure_packed_lazy)
  signed char bky[4][DBM_MAX_TAPS], bkx[4][DBM_MAX_TAPS], bdy[4][DBM_MAX_TAPS], bdx[4][DBM_MAX_TAPS];
};

struct dbm_model {
  dbm_ctx* ctx = nullptr;
  int type = 0;  // 0 generator, 1 discriminator
  std::vector<Tensor> tensors;
  std::map<std::string, int> index;
  float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
  size_t nparam = 0;
  float* pers = nullptr;
  size_t npers = 0;
  double alpha = 1.6e-4, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
  long adam_t = 0;
  int* d_adam_skipped = nullptr;  // device counter of optimizer launches that were no-ops (dbm_ctx::dev_err_flag was set)
  bool adam_ready = false;
  // a persistent-kernel time-out was handled while this model's gradient arena held (or may have held) the sums of a void
  // backward pass: dbm_adam_update answers status 9 until the arena has been cleared (dbm_model_cleargrads, or the cleargrads
  // inside the step entry points) -- whichever call observed the event, and however many host-synchronising calls lie between
  bool grads_void = false;
  // a backward pass has been enqueued into this model's gradient arena since it was last cleared (set by Generator / Discriminator::backward,
  // reset by mark_grads_cleared): a time-out observed while the arena is still clean voids nothing
  bool grads_touched = false;
  bool packed_dirty = true;
  long param_version = 0;  // bumped by every write to the parameter arena
  long packed16_version = -1;  // param_version the bf16 forward images were built from
  bool use_bf16 = false;       // fwd_desc hands out the bf16 images (set around a DBM_BF16 forward)
  void ensure_packed_bf16();
  std::vector<IgLayer> layers;
  PackJob* d_pack_jobs = nullptr;  // device job table of the one-launch weight repack: the FORWARD images (IgLayer::wf)
  int n_pack_jobs = 0, n_pack_blocks = 0;
  // The data-gradient images (IgLayer::wb) are first read by the NEXT backward pass, not by the forward pass that follows an update --
  // in dbm_train_iteration the discriminator's eval-mode pass right behind its update: they have their own table and are rebuilt by
  // ensure_packed_bwd (head of the next iteration, side stream; every backward entry point calls it as well).  DBM_PACK_SPLIT=0: one
  // launch builds both, as before round 5.
  PackJob* d_bwd_jobs = nullptr;
  int n_bwd_jobs = 0, n_bwd_blocks = 0;
  bool bwd_dirty = true;
  void ensure_packed_bwd(hipStream_t on = nullptr);
  PackJob* d_lazy_jobs = nullptr;  // the same for the layers marked lazy
  int n_lazy_jobs = 0, n_lazy_blocks = 0;
  bool pack_tables_built = false;
  long lazy_version = -1;          // param_version the lazy layers' images were built from
  virtual ~dbm_model();
  int add_tensor(const std::string& key, std::vector<int64_t> shape, int kind);
  void alloc_arenas();
  float* P(int ti) const { return params + tensors[ti].off; }
  float* G(int ti) const { return grads + tensors[ti].off; }
  float* S(int ti) const { return pers + tensors[ti].off; }
  int tid(const std::string& key) const;
  int add_iglayer(const std::string& name, int O, int C, int K, int stride, int pad, bool bias, bool as_1x1 = false);
  void ensure_packed(hipStream_t on = nullptr);  // rebuild the packed weight images if the parameters changed
  void ensure_packed_lazy(hipStream_t on = nullptr);  // ... including the layers marked lazy
  virtual void pack_extra(hipStream_t) {}        // model-specific images, same launch point
  // helpers building descriptors
  ConvDesc fwd_desc(const IgLayer& L, const float* x, long xsn, int Hin, int Win, int ups, float* y, long ysn, int N) const;
  // run_dgrad's `base` for the gradient dy (image stride dysn) -> gx (gxsn): zeroed, s1 = s2 = 1; the caller adds accumulate / mask* / r1*
  static ConvDesc dgrad_desc(const float* dy, long dysn, float* gx, long gxsn, int N);
  // reps (op-level tests): one report per launch made, in launch order
  void run_dgrad(const IgLayer& L, ConvDesc base, int Hin_fwd, int Win_fwd, hipStream_t s = nullptr,
                 std::vector<ConvLaunchReport>* reps = nullptr) const;
  // weight gradient of layer L into its own gradient tensors; run_wgrad queues it on `batch` (launched later, all layers at once) or runs
  // it immediately
  WgradDesc wgrad_desc(const IgLayer& L, const float* x, long xsn, int Hin, int Win, int ups, const float* dy, long dysn, int OH, int OW,
                       int N, float scale) const;
  void run_wgrad(const IgLayer& L, const float* x, long xsn, int Hin, int Win, int ups, const float* dy, long dysn,
                 int OH, int OW, int N, float scale, WgradBatch* batch = nullptr) const;
};

// ---- the deformable layers' launch sequences (deform_layer.hip): one copy for Generator::forward / backward and the op-level entry points ----
// Which forms a deformable layer of (C, O) channels takes on an H x W plane.  The only reader of DBM_DEFORM1_PREMUL, DBM_DEFORM1_PREMUL_BWD
// and DBM_DEFORM_WGRAD_FUSED.
struct DeformForms {
  bool fwd_fused;    // the sampler fused into the GEMM, fed from the channels-last input (else: sample matrix + GEMM / GEMV)
  bool fwd_packed;   // the forward reads the layer's packed image (IgLayer::wf); else the OIHW tensor itself
  bool bwd_fused;    // the fused backward kernels + the CSR input-gradient gather (else: launch_deform_backward on the sample matrix)
  bool premul;       // O <= 16 forward: the multiplication before the sampler (needs the z scratch)
  bool premul_bwd;   // 64 -> 1 backward in premultiplied form, when the forward's z planes are there
  bool wgrad_fused;  // 64 -> 64 weight gradient with the sampler fused in (no sample matrix)
};
DeformForms deform_layer_forms(int C, int O, int H, int W);
// y (N, O, H, W) = [lrelu](W * sample(x, off) + b).  Fused: reads xt (channels-last input); yt (channels-last output), col (the sample
// matrix as a by-product) and z (N * 9 * O * H * W floats: the premultiplied form) are optional.  Unfused: reads x, col is required scratch.
// L: the layer's packed images where f.fwd_packed (the unfused GEMM takes its bias from there); w / bias: the OIHW tensor and the bias.
void deform_layer_forward(const dbm_model& m, const IgLayer* L, const DeformForms& f, const float* x, const float* xt, const float* off,
                          long offsn, const float* w, const float* bias, float* y, float* yt, float* col, float* z, int N, int C, int H,
                          int W, int O, int act, hipStream_t s);
// Backward of the C -> 1 layer: gx and goff[:, 0:18] overwritten, gw (C * 9) / gb accumulated.  Fused forms: xt, partial
// (deform_bwd1_partial_floats), csr_ws (deform_csr_workspace_floats; lists_built: its lists are final), z (the forward's premultiplied
// planes or null) and Gt (N * 9 * H * W floats, with z); the gathering form's offset / weight gradients go to s_goff.  Unfused: x and the
// sample matrix col, csr_ws of deform_backward_workspace_floats floats (null where that is 0); the weight gradient goes to s_wgrad.
void deform1_backward(const DeformForms& f, const float* x, const float* xt, const float* off, long offsn, const float* w, const float* gy,
                      const float* z, const float* col, float* gx, float* goff, float* gw, float* gb, float* partial, float* csr_ws,
                      float* Gt, bool lists_built, int N, int C, int H, int W, hipStream_t s, hipStream_t s_goff, hipStream_t s_wgrad);
// Data and offset gradients of the 64 -> 64 layer L (1x1 view; ensure_packed_bwd done): gcol (N, C * 9, H, W) scratch, gx and goff[:, 0:18] overwritten
// (csr_ws: deform_csr_workspace_floats floats for the fused form, deform_backward_workspace_floats for the unfused one)
void deform64_backward_data(const dbm_model& m, const IgLayer& L, const DeformForms& f, const float* x, const float* xt, const float* off,
                            long offsn, const float* gy, float* gcol, float* gx, float* goff, float* csr_ws, bool lists_built, int N, int H,
                            int W, hipStream_t s);
// ... and its weight gradient, gw / gb accumulated: sampler-fused from xt on `s` (partial: deform_wgrad64_partial_floats), or from the sample
// matrix col through the 1x1 form, queued on `batch` or launched on `s`
void deform64_wgrad(const dbm_model& m, const IgLayer& L, const DeformForms& f, const float* xt, const float* col, const float* off, long offsn,
                    const float* gy, float* gw, float* gb, float* partial, int N, int H, int W, hipStream_t s, WgradBatch* batch);

// ---- the input block's launch sequences (generator.hip): one copy for Generator::forward / backward and the op-level entry points ----
// DeepbedmapInputBlock's tensors and layers inside a model: conv_on_X, conv_on_W1, conv_on_W2, conv_on_W3.
struct InputBlockIds {
  int T[4][2];                  // (W, b) tensor ids
  int L[4] = {-1, -1, -1, -1};  // W1 / W2 branches: the layers that run them as im2col + GEMM on the MFMA kernels (1x1 view)
};
// Registers the four convolutions `prefix + conv_on_*` (tensors in save_npz order, then the two wide branches' layers) in m.
InputBlockIds add_input_block(dbm_model& m, const std::string& prefix);
enum InputBlockForm { IN_LAYERWISE = 0, IN_FUSED = 1, IN_ROWS = 2 };
// The form the block takes on H x W tiles for these W1 / W2 pointers.  gemm_bf16: the wide branches' GEMMs multiply in bf16 (the sweep
// with bit 1 of DBM_BF16_FP32_LAYERS cleared): layer-wise only.  The only reader of DBM_INPUT_FUSED.
InputBlockForm input_block_form(int H, int W, const float* w1, const float* w2, bool gemm_bf16);
// y (N, 128, (H-2)(W-2)), image stride ysn; yt (IN_ROWS only, or null): the same concat channels-last INSTEAD of y.  IN_LAYERWISE writes
// the wide branches' im2col images colW1 / colW2 (N * CinP * plane floats each); the other forms leave them alone.
void input_block_forward(const dbm_model& m, const InputBlockIds& ib, InputBlockForm form, int N, int H, int W, const float* x, const float* w1,
                         const float* w2, const float* w3, float* y, long ysn, float* yt, float* colW1, float* colW2, bool gemm_bf16,
                         hipStream_t s);
// The im2col images the wide branches' weight gradients read, rebuilt from the inputs (behind a forward that was not layer-wise).
void input_block_rebuild_cols(const dbm_model& m, const InputBlockIds& ib, int N, int H, int W, const float* w1, const float* w2, float* colW1,
                              float* colW2, hipStream_t s);
// Weight / bias gradients into m's gradient arena from g (N, >= 128, plane), image stride gsn: the wide branches as 1x1 layers over
// their im2col images, queued on `batch` ...
void input_block_queue_wgrads(const dbm_model& m, const InputBlockIds& ib, int N, int H, int W, const float* colW1, const float* colW2,
                              const float* g, long gsn, WgradBatch* batch);
// ... and the two single-channel 3x3 branches, launched on s (no scratch: one workgroup per gradient element)
void input_block_small_wgrads(const dbm_model& m, const InputBlockIds& ib, int N, int H, int W, const float* x, const float* w3, const float* g,
                              long gsn, hipStream_t s);

// Everything one forward / backward pass of the generator leaves behind or works in: activations, gradients, scratch, the record of
// the retained graph and the batches planned over these buffers.  Allocates nothing until a pass sizes it (Generator::ensure_ws).
struct GenWorkspace {
  int N = 0, H = 0, W = 0;
  bool train = false;
  bool have_graph = false;
  // what the retained graph was computed from (opt-in reuse of the D-step's generator forward by the G-step)
  long graph_version = -1;
  long graph_epoch = -1;   // dbm_ctx::data_epoch at the time of that forward
  const float* graph_in[4] = {nullptr, nullptr, nullptr, nullptr};
  bool col_stale = false;   // the retained forward ran the fused input block: colW1 / colW2 are rebuilt by backward()
  const float* bw_in[4] = {nullptr, nullptr, nullptr, nullptr};  // forward inputs, needed by the input-block wgrad
  static const int NWB = 7;
  int wbs_groups = -1;  // trunk groups the batches below were planned for
  WgradBatch wbs[NWB];  // batched weight gradients: tail, 5 trunk groups, pre-residual + input block (launched on the side stream)
  DevBuf colW1, colW2;  // im2col images of the input block's W1 / W2 branches
  std::vector<DevBuf> cat, dA;
  DevBuf in_x, in_w1, in_w2, in_w3, a0, a3, a41, a42, off1, off2, col1, col2, a51, yout;
  DevBuf csr_ws;       // sampling lists of the deformable layers' input-gradient gather (deform_csr_build_kernel)
  // The lists depend on the layers' offsets only.  forward(..., csr_early) marks the two offset tensors (ev_off), prebuild_csr(aux)
  // builds both lists on `aux` beside the generator's loss (the 64 -> 64 layer's in csr_ws, the 64 -> 1 layer's in csr_ws2) and
  // backward() only waits for them (ev_csr) instead of building them on its own path.
  DevBuf csr_ws2;
  bool csr_marked = false, csr_prebuilt = false;
  hipEvent_t ev_off[2] = {nullptr, nullptr}, ev_csr = nullptr;
  DevBuf dw2_partial;  // per-workgroup partial sums of final_conv_layer2's weight gradient (deform_bwd1_fused_kernel)
  DevBuf dw1_partial;  // per-workgroup partial tiles of final_conv_layer1's weight gradient (deform_wgrad64_fused_kernel)
  DevBuf zdef;        // the last layer's premultiplied tap planes (N, 9 * out_ch, 4H, 4W): deform1_premul_kernel
  bool a42t_written = false;  // forward(): post_upsample_conv_layer_2 wrote the channels-last twin of its output itself
  bool zdef_kept = false;  // ... of the retained forward pass (the 64 -> 1 layer's backward in premultiplied form reads them)
  DevBuf gt2;         // backward: the transposed sampler applied to gy, (N, 9, 4H, 4W)
  DevBuf a42t, a51t;  // channels-last copies of the deformable layers' inputs (what the fused sampler gathers from)
  // bf16 sweep mode on large planes (conv_cl16.hip): the dense block's concat as NHWC bf16 (two buffers in ping-pong, 192
  // channels per pixel) and the 64-channel residual stream as NHWC fp32 (block input, block output, RRDB input)
  DevBuf catb[2], resb[4];
  DevBuf a3t, a41t;  // NHWC fp32 inputs of the two upsampling convolutions in the sweep's split-bf16 tail (conv_cl16x3_kernel)
  DevBuf a0t;        // the input block's 128-channel concat channels-last (the split-bf16 pre-residual convolution of the sweep)
  DevBuf a1t;        // NHWC fp32 copy of the trunk's input (the post-residual convolution's skip operand in that tail)
  DevBuf g_a0, g_a3, g_u1, g_z41, g_u2, g_a42, goff1, goff2, gcol, g_a51, g_y;
  // hand-off granules of the persistent trunk kernels and the launch counter they are stamped with: one set per workspace
  unsigned long long* tf_inbox = nullptr;
  int tf_epoch = 0;
  int slot(int j) const { return train ? j : (j == 0 ? 0 : 1 + ((j - 1) & 3)); }
  GenWorkspace() = default;
  GenWorkspace(const GenWorkspace&) = delete;
  ~GenWorkspace();
};

struct Generator : dbm_model {
  int n_rrdb = 12, out_ch = 1;
  float rs = 0.1f;
  // layer indices into `layers`
  int L_pre, L_post, L_up1, L_up2, L_off1, L_def1, L_off2;
  std::vector<int> L_rdb;  // nrdb*5
  InputBlockIds in_ids;    // input block: tensor ids, and the W1 / W2 branches' layers (im2col + GEMM on the MFMA kernels)
  int T_def2W, T_def2b;
  // Two workspaces on the one set of parameters and weight images.  ws[0] serves every single pass; ws[1] holds the G-step's own
  // retained forward, enqueued while the D-step's discriminator passes are still running (dbm_discriminator_step's prefetch flag,
  // dbm_train_iteration).  NOTE the library never has more than FOUR streams busy at once (main, side, chain[0], chain[1]): with
  // a fifth, streams share a hardware queue and independent chains serialise (measured: every phase of the step 2x slower).
  GenWorkspace ws[2];
  hipEvent_t ev_prefetch = nullptr;  // ws[1]'s fakes are final
  hipEvent_t ev_pack[3] = {nullptr, nullptr, nullptr};  // pack_extra: main stream reached the repack / forward streams built / backward streams built
  // fused 9x9 trunk (trunk_fused.hip, trunk_fused_bwd.hip): per-wavefront weight streams
  float* tf_wstream = nullptr;
  float* tf_bstream = nullptr;
  float* tf_bwd_wstream = nullptr;   // transposed / tap-flipped streams of the fused data-gradient chain
  const float** tf_wsrc = nullptr;   // device tables of the trunk layers' W / b
  const float** tf_bsrc = nullptr;
  void pack_extra(hipStream_t s) override;
  bool trunk_fused_ok(int h, int w) const;
  ~Generator() override;
  Generator(dbm_ctx* c, int n, float r, int oc);
  // The passes below run in the workspace they are given, on ctx->stream.
  void ensure_ws(GenWorkspace& ws, int N, int H, int W, bool train);
  void record_graph(GenWorkspace& ws, const float* x, const float* w1, const float* w2, const float* w3) const;  // (behind the forward)
  bool has_graph_of(const GenWorkspace& ws, int N, int H, int W, const float* x, const float* w1, const float* w2, const float* w3) const;
  // max_split: image ranges the 9x9 stage may be cut into (1: everything on the caller's stream); csr_early: mark the offsets for
  // prebuild_csr
  void forward(GenWorkspace& ws, int N, int H, int W, const float* x, const float* w1, const float* w2, const float* w3, float* y,
               bool keep, int max_split = 2, bool csr_early = false);
  void prebuild_csr(GenWorkspace& ws, hipStream_t aux);
  // cleared: the gradient arena has just been zeroed on this stream (WgradBatch::cleared_target); use_aux: the deformable layers'
  // offset-gradient kernels may run on chain[0]
  void backward(GenWorkspace& ws, const float* gy, bool cleared = false, bool use_aux = true);
};

struct Discriminator : dbm_model {
  int L_conv[10];  // 1..9 are igemm layers
  int T_c0W, T_c0b, T_bn[10][5];  // gamma, beta, avg_mean, avg_var, N
  int T_l1W, T_l1b, T_l2W, T_l2b;
  struct Cache {
    int N = 0, H = 0, W = 0;
    bool valid = false;
    DevBuf img, h[10], z[10], mean[10], istd[10], l1, out;
    const float* img_src = nullptr;   // the retained pass's input image: the private copy `img`, or the caller's buffer (forward's `borrow`)
    void drop_borrowed() { if (img_src && img_src != img.p) { valid = false; img_src = nullptr; } }
  } cache[2];
  DevBuf bn_coef[2];  // eval-mode passes: [scale | shift] of all nine BatchNorm layers (launch_bn_eval_coeffs), one buffer per cache
                      // slot: two eval-mode passes in flight on different streams never share coefficients
  DevBuf g_h[2][2], g_z[2][10], g_l1[2], g_out, c0_scratch[2];  // per retained graph: the two backward passes overlap
  static const int NWG = 4;
  WgradBatch wbm[NWG];     // the same for BOTH graphs in one launch per group (the fused D-step: twice the work per launch)
  hipEvent_t ev_grp[2][NWG] = {};
  size_t comm_sent_lo = 0, comm_sent_hi = 0;  // gradient range already handed to the exchange by launch_group (this step)
  void exchange_rest(hipStream_t s);  // the rest of the arena to the exchange, then `s` waits for all of it
  void launch_group(int slot, int g, bool merge);
  WgradBatch wb[2][NWG];  // batched weight gradients per retained graph (real / fake batch): layers 9..6, 5..4, 3..2, 1
  Discriminator(dbm_ctx* c);
  // borrow: conv_layer0's weight gradient reads the caller's image buffer directly instead of a private copy -- one 332 KB copy
  // launch less per pass (round 6).  A borrowed image is good for ONE backward pass, which the borrowing call runs itself: the
  // pass drops it, and so does the call's exit (drop_borrowed), whether it returns or throws.
  void forward(int N, int H, int W, const float* img, float* logits, bool bn_train, bool keep, int slot, bool borrow = false);
  void drop_borrowed() { for (Cache& c : cache) c.drop_borrowed(); }
  void prepare_eval_coeffs(int slot, hipStream_t s);
  // merge: the fused steps' two passes (real first, then fake) share one weight-gradient launch per layer group
  void backward(int slot, const float* glogits, bool join = true, bool merge = false);
};
