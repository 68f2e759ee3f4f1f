// Launchers of the non-GEMM kernels (misc.hip, deform_sampler.hip, norm_loss.hip).
#pragma once
#include <cstdlib>
#include "dbm_internal.h"
#include "../../include/dbm.h"   // the block-median size classes are part of the ABI

struct SmallConvDesc {
  const float* x; long xsn; int Cin, Hin, Win;
  const float* w;     // canonical OIHW
  const float* bias;  // may be null
  float* y; long ysn; int Cout, OH, OW;
  int KH, KW, stride, pad;
  int N;
  int act; float slope;
};
// Zeroed, with the input, the k x k layer, N and the output extent filled: what the weight gradient reads.  The forward's callers add
// w, bias, y, ysn, act and slope.
inline SmallConvDesc small_conv_desc(const float* x, long xsn, int Cin, int Hin, int Win, int Cout, int k, int stride, int pad, int N) {
  SmallConvDesc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.xsn = xsn; d.Cin = Cin; d.Hin = Hin; d.Win = Win;
  d.Cout = Cout; d.OH = conv_out_extent(Hin, k, stride, pad); d.OW = conv_out_extent(Win, k, stride, pad);
  d.KH = d.KW = k; d.stride = stride; d.pad = pad; d.N = N;
  return d;
}
void launch_smallcin_conv_fwd(const SmallConvDesc& d, hipStream_t s);
// scratch (optional, smallcin_wgrad_scratch_floats(Cout) floats, private to the launch): the read-dy-once form (partial sums per
// position slice + fold) for one input channel, 3 x 3, stride 1, pad 1, Cout % 8 == 0 on >= 16384 positions; everything else, and
// every call without scratch, takes one workgroup per gradient element.  form_out (op-level tests): 1 = partial + fold, 0 = per element
void launch_smallcin_conv_wgrad(const SmallConvDesc& d, const float* dy, long dysn, float* gW, float* gb, hipStream_t s,
                                float* scratch = nullptr, int* form_out = nullptr);
size_t smallcin_wgrad_scratch_floats(int Cout);

// DeepbedmapInputBlock on the training tile (11 x 11 -> 9 x 9) as one launch (input_block.hip)
struct InputBlockLaunch {
  const float *x, *w1, *w2, *w3;   // (N,1,11,11), (N,1,110,110), (N,2,22,22), (N,1,11,11), contiguous
  const float *wx, *bx;            // conv_on_X: OIHW (32,1,3,3), bias
  const float *wf1, *b1;           // conv_on_W1: packed forward image [900 (+pad)][32] (IgLayer::wf), bias
  const float *wf2, *b2;           // conv_on_W2: [72 (+pad)][32]
  const float *w3w, *b3;           // conv_on_W3: OIHW
  float* y; long ysn;              // the 128-channel concat (N, 128, plane)
  float* yt;                       // rows form only: the same concat channels-last (N * plane, 128) INSTEAD of y (null: y)
  int N;
};
bool input_block_fused_ok(int H, int W);
void launch_input_block_fused(const InputBlockLaunch& a, hipStream_t s);
// ... on large planes (H x W inputs, the sweep's crops): 32 positions of one output row per workgroup, no im2col image
bool input_block_rows_ok(int H, int W);
void launch_input_block_rows(const InputBlockLaunch& a, int H, int W, hipStream_t s);
void launch_im2col(const float* x, float* col, int N, int Cin, int Hin, int Win, int KH, int KW, int stride, int OH, int OW,
                   int KP, hipStream_t s);
// the sampler, its backward, the CSR sampling lists and their gathers, the 576 -> 1 GEMV: deform_sampler.hip
void launch_deform_sample(const float* x, const float* off, float* col, int N, int C, int H, int W, long offsn, hipStream_t s);
void launch_deform_backward(const float* x, const float* off, const float* gcol, const float* w1o, const float* gy,
                            float* gx, float* goff, int N, int C, int H, int W, long offsn, hipStream_t s, float* ws);
// the floats of list workspace `ws` it needs (0: none; in deterministic mode a plane past its LDS kernels sorts its lists in global memory)
size_t deform_backward_workspace_floats(int N, int C, int H, int W);
// sampler fused into the GEMM (deform_fwd.hip, deform_window.hip; backward: deform_bwd.hip): no column matrix.  C == 64, O == 64 (w = packed [576][64] image) or 1 (w = OIHW).
// xt = the layer input channels-last (N * H * W, 64); yt (optional, O == 64) = the output channels-last as well;
// colout (optional, O == 64) = the sample matrix (N, 576, H, W) as a by-product (a retained pass: the weight gradient reads it)
size_t deform_x3_packed_elems();   // bf16 elements of the split-bf16 weight image of a 64 -> 64 deformable layer
void launch_pack_deform_x3(const float* w_oihw, void* dst, hipStream_t s);
void launch_deform_conv64_x3(const float* xt, const float* off, const void* wx, const float* bias, float* y, float* yt, int N, int H, int W,
                             long offsn, int act, float slope, hipStream_t s, int window = -1);
bool deform_conv_fused_ok(int C, int O);
void launch_nchw_to_nhwc64(const float* x, float* xt, int N, int plane, hipStream_t s);
void launch_deform_conv_fused(const float* xt, const float* off, const float* w, const float* bias, float* y, float* yt, float* colout,
                              int N, int C, int H, int W, long offsn, int O, int act, float slope, hipStream_t s, float* z = nullptr);
// weight gradient of the 64 -> 64 deformable layer with the sampler fused in (no sample matrix): gw (64, 64, 3, 3) / gb (64 or null) += ...
size_t deform_wgrad64_partial_floats(int N, int H, int W);
void launch_deform_wgrad64_fused(const float* xt, const float* off, const float* gy, float* gw, float* gb, float* partial, int N, int H, int W,
                                 long offsn, hipStream_t s);
void launch_deform_bwd64_fused(const float* xt, const float* off, const float* wb, const float* gy, float* gcol, float* goff, int N, int H,
                               int W, long offsn, hipStream_t s);
size_t deform_bwd1_partial_floats(int N, int H, int W);
// the 64 -> 1 layer's backward in the premultiplied form (round 5): z = the forward's premultiplied planes (N, 9, plane), Gt = scratch of
// N * 9 * plane floats, csr_ws = deform_csr_workspace_floats floats; goff and gx (N, 64, plane) overwritten, gw / gb accumulated
void launch_deform_bwd1_premul(const float* xt, const float* off, const float* w, const float* gy, const float* z, float* goff, float* gx,
                               float* gw, float* gb, float* partial, float* csr_ws, float* Gt, int N, int H, int W, long offsn,
                               hipStream_t s, bool lists_built = false);
void launch_deform1_premul(const float* xt, const float* w, float* z, int N, int H, int W, int O, hipStream_t s);
void launch_deform_csr_gather1(const float* off, const float* gy, float* G, int N, int H, int W, long offsn, hipStream_t s, float* ws,
                               bool lists_built = false);
// the sampling lists alone (what launch_deform_csr_gather1 / launch_deform_input_grad build first unless told `lists_built`): they depend on
// the offsets only, so a retained forward can have them built beside its own tail instead of inside the backward pass
bool deform_csr_lists_ok(int C, int H, int W);
void launch_deform_csr_build(const float* off, float* ws, int N, int H, int W, long offsn, hipStream_t s);
void launch_deform_bwd1_fused(const float* xt, const float* off, const float* w, const float* gy, float* goff, float* gw, float* gb,
                              float* partial, int N, int H, int W, long offsn, hipStream_t s);
bool deform_input_grad_ok(int C, int H, int W);
// ws (deform_csr_workspace_floats floats): the sampling lists are built once per (image, tap) there and a register-only kernel gathers
size_t deform_csr_workspace_floats(int N, int H, int W);
void launch_deform_input_grad(const float* off, const float* gcol, const float* w1o, const float* gy, float* gx, int N, int C, int H, int W,
                              long offsn, hipStream_t s, float* ws, bool lists_built = false);
void launch_gemv_cols(const float* col, const float* w, const float* bias, float* y, int N, int K, int plane, hipStream_t s);
void launch_gemv_cols_wgrad(const float* col, const float* gy, float* gw, float* gb, int N, int K, int plane, hipStream_t s);
void launch_sumpool2(const float* g, const float* mask, float* out, long nc, int H, int W, float slope, hipStream_t s);

// ---- norm_loss.hip ----
// BatchNorm (training): per-channel batch statistics of z [N,C,plane]; writes mean/inv_std, updates running stats,
// then y = lrelu(gamma*(z-mean)*inv_std + beta).
// The six kernel forms of training-mode BatchNorm; bn_train_form is the ONE selector (both launchers and dbm_op_batchnorm_train*'s
// form_out go through it; its only inputs are bn_reg_slots / bn_flat_slots and the plane >= 64 && C <= 256 split of the general kernels).
enum BnForm {
  BN_FORM_REG2 = 0,   // bn_train_*_reg_kernel<2>: <= 64 images, planes of 64..128 positions, <= 256 channels
  BN_FORM_REG6 = 1,   // bn_train_*_reg_kernel<6>: ... planes of 129..384 positions
  BN_FORM_FLAT1 = 2,  // bn_train_*_flat_kernel<1>: N * plane <= 256 (planes < 64 positions or > 256 channels)
  BN_FORM_FLAT4 = 3,  // bn_train_*_flat_kernel<4>: N * plane <= 1024
  BN_FORM_WIDE = 4,   // bn_train_*_kernel<1024>: planes >= 64 positions, <= 256 channels (register-cached for <= 64 images of <= 512 positions)
  BN_FORM_GENERAL = 5 // bn_train_*_kernel<256>: everything else
};
BnForm bn_train_form(int N, int C, int plane);
void launch_bn_train_fwd(const float* z, float* y, const float* gamma, const float* beta, float* mean, float* inv_std,
                         float* avg_mean, float* avg_var, int N, int C, int plane, float eps, float decay, float slope,
                         hipStream_t s, const int* hold = nullptr);  // hold: device word; non-zero = no running-average update
struct BnEvalJobs {   // every BatchNorm layer of a model: layer l covers elements [start[l], start[l + 1]) of scale / shift
  static const int MAXL = 12;
  int n, total;
  int start[MAXL + 1];
  const float* gamma[MAXL]; const float* beta[MAXL]; const float* avg_mean[MAXL]; const float* avg_var[MAXL];
  float* scale; float* shift;
};
void launch_bn_eval_coeffs(const BnEvalJobs& jobs, float eps, hipStream_t s);
// backward through lrelu + BN(train): gz = d loss/d z ; ggamma/gbeta accumulated (+=)
void launch_bn_train_bwd(const float* z, const float* gh, const float* gamma, const float* beta, const float* mean,
                         const float* inv_std, float* gz, float* ggamma, float* gbeta, float* scratch, int N, int C,
                         int plane, float slope, hipStream_t s);
// Linear layers of the discriminator head (tiny), backward: gx[n][k] = sum_o gyz[n][o] W[o][k]; gW[o][k] += sum_n gyz[n][o] x[n][k]; gb[o] += sum_n gyz[n][o]
// where gyz = gy * lrelu'(y) if y_act != null else gy
void launch_linear_bwd(const float* x, const float* W, const float* gy, const float* y_act, float* gx, float* gW,
                       float* gb, int N, int K, int O, float slope, hipStream_t s);
// the discriminator's head (linear_1 -> LeakyReLU -> linear_2) as one launch per pass; bitwise the two-launch results
void launch_disc_head_fwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, float* l1, float* logits,
                          int N, int K, int O, float slope, hipStream_t s);
bool disc_head_bwd_fused_ok(int N, int O);
void launch_disc_head_bwd(const float* x, const float* W1, const float* W2, const float* glogits, const float* l1, float* gx, float* gW1,
                          float* gb1, float* gW2, float* gb2, int N, int K, int O, float slope, hipStream_t s);
// The head's backward sequence (Discriminator::backward and dbm_op_disc_head_backward both run THIS): the fused launch if its masked
// gradient fits the LDS, else linear_2's then linear_1's launch_linear_bwd through g_l1 (N x O floats of scratch, read by nothing else).
// Returns whether the fused form ran.
bool disc_head_backward(const float* x, const float* W1, const float* W2, const float* glogits, const float* l1, float* g_l1, float* gx,
                        float* gW1, float* gb1, float* gW2, float* gb2, int N, int K, int O, float slope, hipStream_t s);

// RaGAN discriminator loss (srgan_train.py:960-1009) on N real + N fake logits.
// out[0] = loss, out[1] = binary accuracy (train_eval_discriminator :1156-1158); g_real/g_fake may be null.
// real_targets / fake_targets (device int32[N], may be null): per-sample targets (-1 = ignored) instead of the constants.
void launch_ragan_loss(const float* real, const float* fake, int N, int real_target, int fake_target, float* out,
                       float* g_real, float* g_fake, hipStream_t s, const int* real_targets = nullptr,
                       const int* fake_targets = nullptr);
// mean SSIM's per-image sums (sums[4 n + 2]) for any window_size <= 64 / stride (metric only; the loss kernel is 9 / 1)
void launch_ssim_general(const float* y, const float* t, int N, int H, int W, int ws, int stride, int uniform, float* sums,
                         hipStream_t s);

// Generator loss terms on y_pred vs y_true [N,1,H,W] and x_topo = X[:, :, 1:-1, 1:-1] (srgan_train.py:841-902).
// sums[0..4] = sum|y-t|, sum|pool4(y)-x|, sum ssim_map, sum (y-t)^2, (unused); gy (may be null) receives
// cw*dL1 + tw*dTopo - sw*dSSIM.  X is the full [N,1,H/4+2,W/4+2] input tile.
void launch_gen_loss(const float* y, const float* t, const float* X, int N, int H, int W, float cw, float tw, float sw,
                     const float* win1d, float* sums, float* gy, hipStream_t s);

// Adam (Chainer form, srgan_train.py:1043-1048): one fused pass over the flat arenas.
// skip (may be null): device word; while it is non-zero the update is a no-op (a persistent kernel gave up: the
// gradients of this iteration are invalid, parameters and moments must not be touched).  It is sampled once per launch
// into skipped[1] (adam_gate_kernel): an update is all or nothing.
void launch_adam(float* p, const float* g, float* m, float* v, long n, float alpha_t, float one_minus_beta1,
                 float one_minus_beta2, float eps, float gscale, hipStream_t s, const int* skip = nullptr,
                 int* skipped = nullptr);  // skipped[0] counts the no-op launches, skipped[1] is the launch's gate word
void launch_fill(float* p, long n, float v, hipStream_t s);
void launch_clip_min(float* p, long n, float lo, hipStream_t s);  // p = max(p, lo) in place, NaN kept (np.clip)
void launch_gather_rows(const void* src, void* dst, const int* d_idx, int n, size_t row_bytes, hipStream_t s);
int sqdiff_blocks(long n);  // partial sums launch_sqdiff writes to out[0..blocks)
void launch_sqdiff(const float* a, const float* b, long n, float* out, hipStream_t s);

// ---- fused RRDB trunk forward on 9x9 planes (trunk_fused.hip) ----
#define TRUNK_FUSED_MAXCAT 64
struct TrunkFusedLaunch {
  const float* wstream;  // trunk_fused_stream_floats(nrdb) floats, written by launch_pack_trunk_fused
  const float* bstream;  // nrdb * 192 floats
  const float* in;       // (N, 192, 81) concat buffer whose channels 0..63 hold the trunk input
  float* const* cat;     // HOST table of nrdb + 1 concat buffers (training: every layer output is kept), or null
  float* out;            // cat == null: concat buffer receiving the trunk output in channels 0..63
  unsigned long long* inbox;  // trunk_fused_inbox_bytes(images per launch)
  int* err;              // host-mapped word raised when a neighbour never answered (bounded spins)
  int* err_dev;          // the same flag in device memory: the optimizer kernels skip their update while it is set
  int nrdb, nimg, img0, epoch;
  float rs, slope;
  int no_helper = 0;     // 1: never the four-workgroups-per-image form (data-parallel runs: RCCL's kernels need compute units too)
  // Overrides of what the launcher otherwise takes from the environment / the process state (op-level tests: dbm_op_trunk_forward).
  // The defaults mean "as ever"; host side only, the kernels' arguments are the same.
  int tile = 0;          // 27 or 32: the tile form (0: DBM_TRUNK_TP)
  int helper = -1;       // 1 / 0: ask for / never the helper form, whatever the pass keeps (-1: DBM_TRUNK_HELPER's mask); still TP = 27
                         // only, and only while four workgroups per image fit the device
  int local_st = -1;     // 1 / 0: same-XCD exchange stores may stay in the L2 / agent scope only (-1: trunk_local_stores())
};
// What launch_trunk_fused / launch_trunk_fused_bwd launched (op-level tests), written where the launcher decides.
struct TrunkLaunchReport {
  int form;              // 0 TP = 27, 1 TP = 27 with a helper workgroup per image, 2 TP = 32, 3 the data-gradient chain
  int grid;              // workgroups launched
};
size_t trunk_fused_stream_floats(int nrdb);
size_t trunk_fused_inbox_bytes(int nimg);
void launch_pack_trunk_fused(const float* const* d_wsrc, const float* const* d_bsrc, float* wstream, float* bstream, int nrdb,
                             hipStream_t s);
void launch_trunk_fused(const TrunkFusedLaunch& L, hipStream_t s, TrunkLaunchReport* rep = nullptr);

// ---- fused data-gradient chain of the RRDB trunk on 9x9 planes (trunk_fused_bwd.hip) ----
struct TrunkFusedBwdLaunch {
  const float* wstream;      // trunk_fused_bwd_stream_floats(nrdb), written by launch_pack_trunk_fused_bwd
  const float* gin;          // gradient w.r.t. the output of dense block j1 - 1 (channels 0..63), image stride gin_sn
  long gin_sn;
  float* const* dA;          // HOST table: dA[j] (N, 192, 81), j < nrdb
  const float* const* cat;   // HOST table: forward concat buffers
  const float* g_a3;         // (N, 64, 81): added to the trunk input gradient at j == 0
  unsigned long long* inbox;
  int* err;
  int* err_dev;
  int nrdb, j0, j1;          // dense blocks j1 - 1 ... j0 (both multiples of 3)
  int nimg, img0, epoch;
  float rs, slope;
  int local_st = -1;         // 1 / 0: as TrunkFusedLaunch::local_st (-1: trunk_local_stores())
};
size_t trunk_fused_xcc_offset(int nimg_alloc);  // granules in front of the XCC_ID table at the end of an inbox buffer
int trunk_local_stores();                       // same-XCD exchange stores stay in the L2 (until the first time-out)
extern bool g_trunk_local_off;                  // ... until a persistent kernel has timed out once in this process
size_t trunk_fused_bwd_stream_floats(int nrdb);
void launch_pack_trunk_fused_bwd(const float* const* d_wsrc, float* wstream, int nrdb, hipStream_t s);
void launch_trunk_fused_bwd(const TrunkFusedBwdLaunch& L, hipStream_t s, TrunkLaunchReport* rep = nullptr);

// ---- sync_batch_stats (norm_loss.hip): BatchNorm / RaGAN statistics over the global batch of a data-parallel run ----
void launch_bn_sync_stats(const float* z, float* buf, int N, int C, int plane, hipStream_t s);
void launch_bn_sync_fwd_apply(const float* z, float* y, const float* gamma, const float* beta, const float* buf, float* mean,
                              float* inv_std, float* avg_mean, float* avg_var, int N, int C, int plane, int world, float eps,
                              float decay, float slope, hipStream_t s, const int* hold = nullptr);
void launch_bn_sync_bwd_sums(const float* z, const float* gh, const float* gamma, const float* beta, const float* mean,
                             const float* inv_std, float* buf, float* ggamma, float* gbeta, int N, int C, int plane, float slope,
                             hipStream_t s);
void launch_bn_sync_bwd_apply(const float* z, const float* gh, const float* gamma, const float* beta, const float* mean,
                              const float* inv_std, const float* buf, float* gz, int N, int C, int plane, int world, float slope,
                              hipStream_t s);
void launch_ragan_sync_sums(const float* real, const float* fake, int N, float* buf, hipStream_t s);
void launch_ragan_sync_loss(const float* real, const float* fake, int N, int world, int real_target, int fake_target, float* buf,
                            float* out, hipStream_t s);
void launch_ragan_sync_grad(const float* real, const float* fake, int N, int world, int real_target, int fake_target,
                            const float* buf, float* g_real, float* g_fake, hipStream_t s);

// ---- channels-last bf16 3x3 convolution for the trunk of the bf16 area sweep on large planes (conv_cl16.hip) ----
struct ClConvLaunch {
  const void* x; int xc;     // input NHWC bf16 (xc channels per pixel), channels [0, Cin) are read
  int Cin, Cout;             // Cin % 32 == 0, Cout 32 or 64
  const void* w;             // packed by launch_pack_cl16
  const float* bias;
  void* y16; int yc, y0;     // bf16 output (NHWC, yc channels per pixel, first channel y0) or null
  float* y32;                // fp32 output (NHWC, 64 channels per pixel) or null
  const float* r1; float s1; // v = s1 * (acc + bias) + r1 (NHWC fp32, 64 channels), if r1
  const float* r2; float s2; // v = s2 * v + r2, if r2
  int act; float slope;
  int N, H, W;
  const void* zeros;         // >= 16 bytes of device zeros (dbm_ctx::zeros)
};
size_t cl16_packed_elems(int Cin, int Cout);   // bf16 elements of a layer's packed image
void launch_pack_cl16(const float* w_oihw, void* dst, int O, int C, hipStream_t s);
// conv_cl16's epilogue reaches one image's operands through 32-bit byte offsets: 256 bytes per pixel (fp32 64 channels) and, for a bf16
// channels-last output of yc16 channels (0: none), 2 * yc16 bytes per pixel must stay below 2^31 per image plane
bool conv_cl16_plane_ok(long plane, int yc16);
void launch_conv_cl16(const ClConvLaunch& L, hipStream_t s);
// (N, 64, plane) fp32 [image stride xsn] -> NHWC fp32 (res, may be null) and NHWC bf16 channels 0..63 of a buffer with `ac`
// channels per pixel (act, may be null); and back
void launch_nchw_to_cl(const float* x, long xsn, float* res, void* act, int ac, int N, int plane, hipStream_t s, int nch = 64);
void launch_cl_to_nchw(const float* res, float* y, long ysn, int N, int plane, hipStream_t s, int nch = 64);

// split-bf16 (three bf16 MFMAs per product: 2^-16 operand precision) 3x3 convolution on NHWC fp32 activations: the layers on
// the signal path of the bf16 sweep (upsampling and offset convolutions)
struct ClX3Launch {
  const float* x; int xc;    // input NHWC fp32 (xc channels per pixel), channels [0, Cin) are read
  int Cin, Cout;             // Cin % 16 == 0, Cout <= 64
  int ups;                   // 1: x is the (H / 2, W / 2) plane (nearest x2 folded in)
  const void* w;             // packed by launch_pack_cl16x3
  const float* bias;
  float* y32; int yc;        // NHWC fp32 output (yc channels per pixel; all 32 * ceil(Cout / 32) channels are written) or null
  const float* r1; int r1c;  // optional residual, NHWC fp32 (r1c channels per pixel): v = conv + bias + r1 (before the activation)
  void* y16; int y16c;       // optional second output: the same values as bf16, NHWC with y16c channels per pixel (channels [0, 32 MT))
  float* yp; long ysn; int ypc;  // channel planes yp[n * ysn + co * H * W + pixel], co < ypc, or null
  int act; float slope;
  int N, H, W;               // output plane
};
size_t cl16x3_packed_elems(int Cin, int Cout);
void launch_pack_cl16x3(const float* w_oihw, void* dst, int O, int C, hipStream_t s);
void launch_conv_cl16x3(const ClX3Launch& L, hipStream_t s);

// Grid sampling along survey tracks (track.hip; dbm_grid_track): the float32 grid (H, W) evaluated at n float64 points (x, y[, z])
// with 64-bit offsets; z_out (n doubles) and part (6 doubles per workgroup: the error moments, folded into stats[6]) may be null
struct TrackLaunch {
  const float* grid;
  long H, W;
  double x0, y0, dx, dy;
  double tlo, thi, slo, shi;   // the domain in node units (registration)
  const double* points;        // (n, ncol), ncol 2 or 3 (part needs 3)
  long n;
  int ncol, interp;            // 0 nearest, 1 bilinear, 2 bicubic
  double threshold;
  double* z_out;
  double* part;
};
int grid_track_blocks(long n);   // workgroups of the sampling launch (depends on n only): partials needed
void launch_grid_track(const TrackLaunch& a, double* stats, hipStream_t s);

// The errors of one dbm_grid_track call (track_dist.hip; dbm_track_error_quantiles, dbm_track_error_histogram): e_i = z_interp[i] -
// points[3 i + 2], finite ones only, -0.0 as +0.0.  Quantiles: `count` probabilities (host) -> out (device), NumPy's method="linear" on
// exact order statistics (radix select, 8 passes over the points whatever `count`).  Histogram: np.histogram's uniform-bin rule with
// the caller's bins + 1 edges (host, copied into ws) -> counts (device, int64).  ws: track_*_workspace() bytes, 256-byte aligned.
struct TrackErrors {
  const double* points;
  const double* z_interp;
  long n;
};
size_t track_quantiles_workspace();
size_t track_histogram_workspace(int bins);
void launch_track_error_quantiles(const TrackErrors& a, const double* probs, int count, double* out, void* ws, hipStream_t s);
void launch_track_error_histogram(const TrackErrors& a, const double* edges_host, int bins, long long* counts, void* ws, hipStream_t s);

// Gridline -> pixel registration (track.hip; dbm_grid_to_pixel, `grdsample -T`): out (H - 1, W - 1) = the bicubic interpolant of
// launch_grid_track (same weights, ghost nodes, NaN / threshold rule) at the cell centres (c + 1/2, r + 1/2), rounded to float32 once
void launch_grid_to_pixel(const float* in, long H, long W, double threshold, float* out, hipStream_t s);

// Cutting tiles from a resident raster (tile.hip; dbm_grid_tile): out[k * out_stride + r * out_w + c] for n windows of (out_h, out_w).
// mode 1: windows = n x (left, bottom, right, top) doubles, bilinear at np.linspace coordinates of resolution res; mode 0: windows =
// n x (row0, col0, row step, column step) int64, a copy (every node inside the raster: checked by the caller).  counts (n ints,
// zeroed by the caller) may be null.
struct TileLaunch {
  const float* grid;
  long H, W;
  double x0, y0, dx, dy;
  const void* windows;         // device
  long n;
  int out_h, out_w, mode;
  double res;
  int has_nodata, has_fill, fill_nan;
  double nodata, nodata_band;  // masked iff |v - nodata| <= nodata_band = 1e-8 + 1e-5 |nodata|
  float fill;
  float* out;
  long out_stride;             // floats between windows, >= out_h * out_w
  int* counts;
};
void launch_grid_tile(const TileLaunch& a, hipStream_t s);
// Gaps of a fine raster filled from a coarse one (tile.hip; dbm_grid_fill_gaps): `a` describes the mode 1 cut of the COARSE raster with
// ONE window (a.windows: host values passed by value in `window`), out_h x out_w = the fine raster; out[i] = fine[i] unless fine[i] is
// NaN or (has_fine_nodata) equals fine_nodata, then the value launch_grid_tile would write at i.  out may be fine.
void launch_grid_fill_gaps(const TileLaunch& a, const double window[4], const float* fine, int has_fine_nodata, float fine_nodata, float* out,
                           hipStream_t s);

// Block reads (dbm_tiff_decode, dbm_chunk_decode).  blocks: n_blocks x 8 int64 on the device = {offset of the block's bytes in the
// upload, their count, rows the block holds, output row of the block's row 0, output column of its column 0, id, row step (chunks:
// +1 / -1; GeoTIFF: 0, not read), 0}.  sample_type: 0 uint8, 1 int16, 2 uint16, 3 int32, 4 float32, 5 float64, 6 int8 (chunks only).
inline int block_sample_bytes(int sample_type) {
  static const int kBytes[7] = {1, 2, 2, 4, 4, 8, 1};
  return kBytes[sample_type];
}

// The stream decoders, one wavefront per block: launch_block_lzw (TIFF 6.0 LZW, tiff_decode.hip) or launch_block_inflate (zlib streams,
// tiff_inflate.hip) decodes streams + offset into stage + b * block_stride and writes status[b]: 0 good, 1 malformed, 2 the decoded
// size is not want = (whole_rows ? whole_rows : rows held) * row_bytes.  whole_rows: 0, or block_h where a block is always stored whole
// (HDF5 chunks) however many rows it holds.
struct StreamDecodeLaunch {
  const uint8_t* streams;
  uint8_t* stage;
  const long* blocks;
  int* status;
  int n_blocks;
  long block_stride;           // bytes between decoded blocks in stage, a multiple of 16, >= block_h * row_bytes
  long row_bytes;              // block_w * bytes per sample
  int whole_rows;
};
void launch_block_lzw(const StreamDecodeLaunch& a, hipStream_t s);
void launch_block_inflate(const StreamDecodeLaunch& a, hipStream_t s);

// GeoTIFF blocks -> a float32 plane (tiff_decode.hip; dbm_tiff_decode).  staged: the blocks were decoded to stage + b * block_stride;
// else the block's decoded bytes lie at stage + offset (8-byte aligned).  launch_tiff_rows changes the decoded bytes in place (the
// predictor) and writes out (out_h, out_w).
struct TiffDecodeLaunch {
  uint8_t* stage;
  const long* blocks;
  int n_blocks, staged;
  long block_stride;           // bytes between staged blocks, a multiple of 16, >= block_h * block_w * bytes
  int block_w, block_h, bytes; // samples per block row, rows of a whole block, bytes per sample
  int sample_type;             // 0..5
  int predictor;               // 1 none, 2 horizontal differencing, 3 floating point
  float* out;
  long out_h, out_w;
};
void launch_tiff_rows(const TiffDecodeLaunch& a, hipStream_t s);
// lzw_decode_lanes with one lane on the host: the decoded size or (size_t)-1 (tools/lzw_twin_check.cpp compares it with dbm_lzw_decode)
size_t tiff_lzw_decode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);
// inflate_lanes with one lane on the host: the decoded size or (size_t)-1 (dbm_inflate; tools/inflate_twin_check.cpp compares it with zlib)
size_t tiff_inflate_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

// Chunks of a netCDF variable -> a float32 plane (nc_chunks.hip; dbm_chunk_decode).  staged: the blocks were inflated to
// stage + b * block_stride; else the block's bytes lie at stage + offset (8-byte aligned).  Row r of a block lands on output row
// e[3] + e[6] * r.
struct ChunkDecodeLaunch {
  const uint8_t* stage;
  const long* blocks;
  int n_blocks, staged;
  long block_stride;           // bytes between staged blocks, a multiple of 16, >= block_h * block_w * bytes
  unsigned groups_per_block;   // nc_chunks_groups_per_block(block_w, block_h)
  int block_w, block_h, bytes; // samples per block row, rows of a whole block, bytes per sample
  int sample_type;             // 0..6
  int shuffle, big_endian;     // HDF5 shuffle over the whole block; the samples' byte order
  int has_fill, has_scale;
  unsigned long long fill_bits;  // the fill in the sample's width
  double scale, offset;
  float* out;
  long out_h, out_w;
};
unsigned nc_chunks_groups_per_block(int block_w, int block_h);
void launch_nc_chunks(const ChunkDecodeLaunch& a, hipStream_t s);

// A float32 plane -> the chunks of a netCDF-4 variable (nc_chunks.hip; dbm_chunk_encode): the inverse of the above.  The call's chunks
// are first .. first + n_blocks - 1, row-major over chunks_x columns of chunks.  Chunk row r of the chunk whose first row is r0 is
// plane row r0 + r (row_step +1) or H - 1 - (r0 + r) (row_step -1: a file whose y ascends); positions beyond the plane are zero
// bytes; the values are the 32-bit patterns; shuffle: byte k of element i goes to k * n + i, n = chunk_h * chunk_w.
struct ChunkEncodeLaunch {
  const float* plane;
  long H, W;
  int chunk_h, chunk_w;
  int row_step, shuffle;
  long first, chunks_x;
  int n_blocks;
  unsigned groups_per_block;   // nc_chunks_groups_per_block(chunk_w, chunk_h)
  uint8_t* raw;
  long raw_stride;             // a multiple of 16, >= chunk_h * chunk_w * 4
};
void launch_nc_chunk_cut(const ChunkEncodeLaunch& a, hipStream_t s);

// Blocks of bytes -> zlib streams with the fixed Huffman code (deflate_encode.hip), one wavefront per block: block b's block_bytes
// bytes at raw + b * raw_stride into slots + b * slot_cap; result[2 b] = the stream's size, result[2 b + 1] = its status word (1: it
// did not fit; size 0), as launch_tiff_lzw_encode.  deflate_slot: the room that always holds a stream (9 bits per byte at most).
// segments != 0 (the bands of a PNG, dbm_png_encode): the blocks are segments of ONE zlib stream -- no header, no Adler-32 in the
// stream; block last_block (-1: none of this launch) ends the stream, holds last_bytes bytes and is written with BFINAL 1, every other
// block ends in an empty stored block -- and segment_words[2 b], [2 b + 1] receive the Adler-32 of block b's bytes and their number.
struct DeflateLaunch {
  const uint8_t* raw;
  size_t raw_stride, block_bytes;
  int n_blocks;
  uint8_t* slots;
  size_t slot_cap;
  uint32_t* result;
  int segments = 0;
  long last_block = -1;
  size_t last_bytes = 0;
  uint32_t* segment_words = nullptr;
};
inline size_t deflate_slot(size_t n) { return n + n / 8 + 16; }
void launch_block_deflate(const DeflateLaunch& a, hipStream_t s);
// deflate_encode_lanes with one lane on the host (png_encode.hip's host writer): framing 0 a whole zlib stream, 1 a middle segment, 2
// the last segment; table: 16 384 entries of scratch; *adler_out (framing 1, 2): the Adler-32 of src[0, n).  Returns the size, 0 if
// cap is too small.
size_t deflate_encode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, uint16_t* table, int framing, uint32_t* adler_out);

// numpy.ndarray.astype(int16) of a float32 on x86-64: truncation to int32 (cvttss2si: NaN and |x| >= 2^31 give INT32_MIN), then the low
// 16 bits -- NaN (the canvas frame that no tile covers), +-inf and out-of-range values become 0.  The one cast of f32_to_i16_kernel
// (tiff_lzw.hip) and tiff_blocks_kernel (tiff_encode.hip).
__device__ inline short dbm_cast_i16(float x) {
  const int v = (x == x && x > -2147483648.f && x < 2147483648.f) ? (int)x : (int)0x80000000;
  return (short)(v & 0xffff);
}

// A float32 plane -> the blocks (strips or tiles) of a GeoTIFF (tiff_encode.hip; dbm_tiff_encode).  The call's blocks are first ..
// first + n_blocks - 1 of the image, row-major over blocks_x columns of blocks.  launch_tiff_blocks writes block b's raw bytes (cast,
// padding, predictor) at raw + b * raw_stride; launch_tiff_lzw_encode encodes them into slots + b * slot_cap (slot_cap bytes of room)
// and writes result[2 b] = the stream's size, result[2 b + 1] = its status word (1: it did not fit; size 0); launch_tiff_pack copies
// n_blocks streams (block b at src + b * src_stride; table = {offset in packed, size} per block, on the device) to their offsets.
struct TiffEncodeLaunch {
  const float* plane;
  long H, W;
  int sample_type;             // 1 int16 (by cast), 4 float32 (the bits): dbm_tiff_decode's numbering
  int bytes;                   // bytes per sample
  int block_h, block_w, tiled; // tiled: blocks are whole (zero padded); else strips of block_w == W, the last one short
  int predictor;               // 1 none, 2 horizontal differencing
  long first, blocks_x;
  int n_blocks;
  uint8_t* raw;
  long raw_stride;             // a multiple of 16, >= block_h * block_w * bytes
  uint8_t* slots;
  size_t slot_cap;
  uint32_t* result;
};
void launch_tiff_blocks(const TiffEncodeLaunch& a, hipStream_t s);
void launch_tiff_lzw_encode(const TiffEncodeLaunch& a, hipStream_t s);
void launch_tiff_pack(const uint8_t* src, size_t src_stride, const unsigned long long* table, int n_blocks, uint8_t* packed, hipStream_t s);
// lzw_encode_lanes with one lane on the host: the encoded size, or 0 if cap is too small (tools/lzw_encode_twin_check.cpp compares it
// with dbm_lzw_encode_tiles)
size_t tiff_lzw_encode_twin(const uint8_t* src, size_t n, uint8_t* dst, size_t cap);

// The overview pyramid of a plane (pyramid.hip; dbm_grid_overviews): `levels` nodata-aware halvings of the plane as a file of
// sample_type holds it, written back to back to out as float32 planes of (H + 1) / 2 x (W + 1) / 2, ... -- three levels per launch.
// nodata: float32(nodata) for float32 files, float(int(nodata)) for int16 files.  pyramid_max_levels: the halvings down to 1 x 1.
struct PyramidLaunch {
  const float* plane;
  long H, W;
  int sample_type;             // 1 int16 (level 0 by dbm_cast_i16, results rounded to even), 4 float32
  float nodata;
  int levels;
  float* out;
};
int pyramid_max_levels(long H, long W);
void launch_grid_overviews(const PyramidLaunch& a, hipStream_t s);

// Colour relief and hillshade of a plane (relief.hip; dbm_grid_relief, dbm_grid_shade_stats): the float32 plane -> out, uint8 (H, W,
// channels).  edges (n_slices + 1 doubles) and colors (6 bytes per slice: the colour at its lower edge, then at its upper edge) are
// DEVICE pointers; bfn holds the colours below the table, above it and of NaN.  shade: the intensity k atan((g - mean) / sigma) of the
// gradient g along (sin_a, cos_a), dy scaled by aspect.  launch_shade_stats leaves {n, mean, sigma} of the defined g in the first three
// doubles of ws (shade_stats_workspace(H, W) bytes); it reads plane, H, W, sin_a, cos_a and aspect only.
constexpr int RELIEF_MAX_SLICES = 2048;
struct ReliefLaunch {
  const float* plane;
  long H, W;
  const double* edges;
  const uint8_t* colors;
  int n_slices, channels, shade;
  uint8_t bfn[9];
  double sin_a, cos_a, aspect, mean, sigma, k;
  uint8_t* out;
};
void launch_grid_relief(const ReliefLaunch& a, hipStream_t s);
size_t shade_stats_workspace(long H, long W);
void launch_shade_stats(const ReliefLaunch& a, void* ws, hipStream_t s);

// Perspective view of a plane (perspective.hip; dbm_grid_perspective, dbm_grid_perspective_host, dbm_grid_minmax; the rule: the head of
// perspective.hip and DESIGN.md 6o): the float32 plane (H, W) and its drape, uint8 (H, W, channels) at the nodes -> out, uint8 (Ho, Wo,
// 4), and hits, int32 (Ho, Wo) or null: the id of the visible triangle, -2 a wall, -1 none.  All DEVICE pointers.  The launch fills
// the block counts and the workspace pointers itself from ws (grid_perspective_workspace(a) bytes; none if H < 2 or W < 2).
// perspective_check_arguments: what the device and the host entry refuse alike; fills the view from the caller's nine doubles.
// launch_grid_minmax leaves {count of finite samples, min, max} (NaN, NaN if the count is 0) in the first three doubles of ws.
struct PerspView {
  double sin_a, cos_a, sin_e, tan_e, level, zfac, sx0, sy0, step;
};
struct PerspLaunch {
  const float* plane;
  long H, W;
  const uint8_t* drape;
  int channels;
  PerspView v;
  long Wo, Ho;
  int facade_on;
  uint8_t facade[4], background[4];
  uint8_t* out;
  int32_t* hits;
  float *max8, *max64, *part, *zrange;   // (the launch's own)
  long n8x, n8y, n64x, n64y;
};
size_t grid_perspective_workspace(const PerspLaunch& a);
void launch_grid_perspective(const PerspLaunch& a, void* ws, hipStream_t s);
void perspective_check_arguments(const char* who, const void* plane, long H, long W, const void* drape, int drape_channels, const double* view,
                                 long Wo, long Ho, const void* background, const void* out, PerspView& v);
// the render on host threads from HOST pointers (no GPU): the plain walk, or with `skipping` the device's own traversal
void perspective_render_host(const PerspLaunch& a, bool skipping, int nthreads);
size_t grid_minmax_workspace(long H, long W);
void launch_grid_minmax(const float* plane, long H, long W, void* ws, hipStream_t s);

// An 8-bit image -> the bands of a PNG's filtered scanlines (png_encode.hip; dbm_png_encode): band b of the call holds the image rows
// (first_band + b) * band_rows ..., each as one filter-type byte and row_bytes filtered bytes (filter 0 None, 1 Sub, 2 Up, from the raw
// image), at raw + b * raw_stride (raw_stride a multiple of 16, >= band_rows * (row_bytes + 1)).  png_check_arguments: what the device
// and the host entry refuse alike; returns the image's number of bands.
struct PngFilterLaunch {
  const uint8_t* image;
  long H, row_bytes;
  int bpp, filter, band_rows;
  long first_band;
  int n_bands;
  unsigned groups_per_band;    // png_groups_per_band(band_rows * (row_bytes + 1))
  uint8_t* raw;
  long raw_stride;
};
unsigned png_groups_per_band(long band_bytes);
void launch_png_filter(const PngFilterLaunch& a, hipStream_t s);
// dbm_png_encode's workspace, carved from ws (data_prims.h's carver; ws == nullptr only measures: `bytes`): the filtered bands, the
// segments' slots, words_per_band bytes of bookkeeping per band, the segments' {Adler-32, length}
struct PngWorkspace {
  uint8_t *raw, *slots;
  uint32_t *words, *segment_words;
  size_t bytes;
};
PngWorkspace png_workspace(void* ws, size_t n_bands, size_t raw_stride, size_t slot_cap, size_t words_per_band);
long png_check_arguments(const char* who, const void* image, long H, long W, int channels, int filter, int band_rows, long first_band, int n_bands,
                         const void* out, size_t out_capacity, const void* sizes, const void* adlers);

// Fully filled windows of a raster (tile.hip; dbm_grid_filled_windows): flags[uly * nx + ulx] = 1 iff no node of rows [uly step, uly step
// + size) x columns [ulx step, ulx step + size) is NaN, rows counted from the north (flip_rows: raster row 0 is the south edge), columns
// from the west (flip_cols).  rowany: rows * nx bytes of scratch.  filled_windows_geometry fills ny, nx, rows, nw, nseg from H, W,
// size, step (size <= FILLED_LDS_BYTES).
constexpr long FILLED_LDS_BYTES = 8192;
struct FilledLaunch {
  const float* grid;
  long H, W;
  int size, step, flip_rows, flip_cols;
  long ny, nx, rows;           // candidate windows; raster rows they cover
  long nw, nseg;               // window columns per workgroup of the row pass, workgroups per row
  unsigned char* rowany;
  unsigned char* flags;
};
void filled_windows_geometry(FilledLaunch& a);
void launch_filled_windows(const FilledLaunch& a, hipStream_t s);

// Rescaling a resident grid (resample.hip; dbm_grid_rescale): the float32 grid (H, W) -> out (out_h, out_w), the scipy.ndimage chain of
// scikit-image's `rescale`: optional int32 cast, min / max for the clip, Gaussian per downscaled axis, cubic B-spline prefilter (order 3),
// linear or cubic evaluation at (o + 0.5) in / out - 0.5, everything mirrored at the edges, float64 until the one final rounding.
// ws: grid_rescale_workspace(a) doubles of scratch (two float64 planes unless order 1 runs unfiltered).
struct RescaleLaunch {
  const float* in;
  long H, W, out_h, out_w;
  int order, anti_aliasing, clip, input_cast;
  float* out;
  double* ws;
};
size_t grid_rescale_workspace(const RescaleLaunch& a);
void launch_grid_rescale(const RescaleLaunch& a, hipStream_t s);

// Rolling-window standard deviation (resample.hip; dbm_grid_rolling_std): population standard deviation of the non-NaN nodes of the
// centred window x window neighbourhood cut at the edges (window odd, 1..63), NaN where there is none
void launch_rolling_std(const float* in, long H, long W, int window, float* out, hipStream_t s);

// Survey point clouds (points.hip; dbm_points_polar_stereographic, dbm_points_region, dbm_points_blockmedian): float64 tables (n, ncol)
// Polar stereographic, variant B, south-pole case: columns 0, 1 (longitude, latitude in degrees) -> (easting, northing), the rest copied;
// e = eccentricity, half_e = e / 2, scale = 2 a k0 / sqrt((1+e)^(1+e) (1-e)^(1-e)), lon0 in radians (host, float64); out may be in
struct ProjLaunch {
  const double* in;
  double* out;
  long n;
  int ncol;
  double e, half_e, scale, lon0, fe, fn;
};
void launch_points_project(const ProjLaunch& a, hipStream_t s);
// region[4] = {floor(xmin / inc) inc, ceil(xmax / inc) inc, floor(ymin / inc) inc, ceil(ymax / inc) inc} over the rows whose x, y[, z] are
// finite, *count = their number (none: four NaNs, 0); ws: points_region_workspace(n) bytes
size_t points_region_workspace(long n);
void launch_points_region(const double* pts, long n, int ncol, double inc, void* ws, double* region, long long* count, hipStream_t s);
// Block medians of (n, 3) rows on the H x W gridline-registered blocks of spacing inc whose north-west node is (xmin, ymax).  Two phases
// with a host read of totals between them: _count fills blk, cnt, off, rowof, the size classes' lists and totals = {non-empty blocks,
// blocks per class}; _select writes table (3 doubles per non-empty block, block-index order), grid and counts (H W each, may be null).
struct BlockMedianLaunch {
  const double* points;
  long n, H, W;
  double xmin, ymax, inc;
  int* blk;            // n: block of each row or -1
  unsigned* perm;      // n: rows, block-contiguous
  unsigned* cnt;       // H W: histogram (counted down to zero by the scatter)
  unsigned* rowof;     // H W: table row of a non-empty block
  unsigned* off;       // H W + 1: first place of each block in perm
  uint2* part;         // per scan tile: (points, non-empty blocks) before it
  unsigned* totals;    // 1 + DBM_BLOCKMEDIAN_CLASSES
  unsigned* lists[DBM_BLOCKMEDIAN_CLASSES];
  double* table;
  float* grid;
  int* counts;
};
size_t blockmedian_workspace(long n, long hw);   // bytes
void blockmedian_carve(BlockMedianLaunch& a, void* ws);
void launch_blockmedian_count(const BlockMedianLaunch& a, hipStream_t s);
void launch_blockmedian_select(const BlockMedianLaunch& a, const unsigned* totals, hipStream_t s);

// Survey text tables (text.hip; dbm_text_count_lines, dbm_text_parse): the bytes of a delimited text file -> the float64 rows that
// pandas.read_csv + dropna keep.  launch_text_structure counts and scans the lines per tile of DBM_TEXT_TILE_BYTES (totals[0], [1] =
// lines, non-blank lines); the host reads them and sizes the candidates' scratch (ncand = non-blank lines behind the first skip1);
// launch_text_parse fills it and scans the flags (totals[2] = smallest byte offset of an offending line or ~0, [3], [4] = rows kept,
// rows with a field the device leaves to the host); launch_text_compact writes table (kept rows, file order) and repair (byte offset,
// final row per such row).  text must be 16-byte aligned.
struct TextPair {
  unsigned long long a, b;
};
struct TextLaunch {
  const unsigned char* text;
  unsigned long long len;
  int sep;                        // the separator byte, or DBM_TEXT_SEP_WHITESPACE
  unsigned long long skip1;       // non-blank lines discarded unparsed (skip + 1)
  int nfields, nuse;              // names; used names
  unsigned long long use_mask;    // bit f: field f is used
  int n_na;                       // the caller's NA strings, packed little-endian
  int na_len[DBM_TEXT_MAX_NA];
  unsigned long long na_lo[DBM_TEXT_MAX_NA], na_hi[DBM_TEXT_MAX_NA];
  TextPair* tiles;                // per tile: (lines, non-blank lines) started there, then the counts in front of the tile
  unsigned long long* totals;     // 5
  unsigned long long* first_error;
  unsigned long long ncand;
  double* rows;                   // ncand x nuse scratch
  unsigned long long* offs;       // ncand: byte offset of the candidate's line
  unsigned char* flags;           // ncand: bit 0 kept, bit 1 needs the host
  TextPair* parts;                // per scan tile of the flags
  double* table;
  long long* repair;
};
long text_tiles(size_t nbytes);
size_t text_structure_workspace(size_t nbytes);
void text_structure_carve(TextLaunch& a, void* ws);
size_t text_parse_workspace(size_t ncand, int nuse);
void text_parse_carve(TextLaunch& a, void* ws);
void launch_text_structure(const TextLaunch& a, hipStream_t s);
void launch_text_parse(const TextLaunch& a, hipStream_t s);
void launch_text_compact(const TextLaunch& a, hipStream_t s);
// The steps behind the read (dbm_text_columns): column c of out = column a[c] of in, plus (op 1) or minus (op 2) column b[c]
struct ColumnsLaunch {
  const double* in;
  double* out;
  unsigned long long n;
  int ncol_in, ncol_out;
  int a[DBM_TEXT_MAX_COLUMNS], op[DBM_TEXT_MAX_COLUMNS], b[DBM_TEXT_MAX_COLUMNS];
};
void launch_text_columns(const ColumnsLaunch& a, hipStream_t s);

// Tension-spline surface through the non-NaN nodes of a float32 raster (surface.hip; dbm_grid_tension_surface), float64 conjugate
// gradients on the device; ws: surface_workspace(H, W) bytes, 256-byte aligned.  surface_solve synchronises the stream, fills info =
// {iterations, |r| / |b|, constraint nodes, free nodes}, always writes out (the last iterate) and returns whether |r| <= tol |b| was
// reached within max_iter; it throws status 1 before writing anything when no node is a constraint.
struct SurfaceLaunch {
  const float* data;
  long H, W;
  double tension, tol;
  int max_iter;
  float* out;
};
size_t surface_workspace(long H, long W);
bool surface_solve(const SurfaceLaunch& a, void* ws, hipStream_t s, double info[4]);
// grid[r, c] = NaN unless a non-NaN node of data lies within `radius` nodes (Euclidean, integer arithmetic) (dbm_grid_distance_mask)
void launch_distance_mask(const float* data, float* grid, long H, long W, int radius, hipStream_t s);

// Nodes inside a buffered polygon set (polygon.hip; dbm_grid_polygon_mask): edges (n, 4) float64 (xa, ya, xb, yb) on the device, 16-byte
// aligned.  polygon_geometry fills the tiling, the nodes' extent and `identity` (coordinates beyond 2^480: no culling, no shortcuts) from
// H, W, x0, y0, dx, dy, buffer; polygon_carve hands out polygon_workspace bytes (256-byte aligned; returns the staging area for a host
// table if asked for).  launch_polygon_cull fills listP / listB / cnt and totals = {proximity edges, parity edges, non-finite edges, wild
// edges, tile bin entries, band bin entries}; the host reads totals, sets nP, nB, identity and -- if it bins -- entries (totals[4] +
// totals[5] indices), then launch_polygon_bin; launch_polygon_classify writes mask (0 / 1, may be null) and NaN into grid (may be null).
constexpr size_t DBM_POLY_WORKSPACE_DEFAULT = (size_t)256 << 20;   // bytes of bin entries above which a call runs unbinned
struct PolyLaunch {
  const double* edges;
  long n, H, W;
  double x0, y0, dx, dy, buffer;
  double gmag, gx0, gx1, gy0, gy1;   // largest magnitude of a node coordinate or the buffer; the nodes' extent
  long tiles_x, tiles_y, nbins;      // node tiles per row, tile rows (= bands); tiles_x tiles_y + tiles_y bins
  unsigned* listP;                   // n: culled proximity edges
  unsigned* listB;                   // n: culled parity edges
  unsigned* cnt;                     // nbins
  unsigned* cursor;                  // nbins
  unsigned* off;                     // nbins + 1
  unsigned* part;                    // per scan tile
  unsigned long long* totals;        // 8
  unsigned* entries;                 // null: unbinned
  int identity;
  unsigned nP, nB;
  unsigned char* mask;
  float* grid;
};
void polygon_geometry(PolyLaunch& a);
size_t polygon_workspace(const PolyLaunch& a, bool stage_edges_too);
double* polygon_carve(PolyLaunch& a, void* ws, bool stage_edges_too);
void launch_polygon_cull(const PolyLaunch& a, hipStream_t s);
void launch_polygon_bin(const PolyLaunch& a, hipStream_t s);
void launch_polygon_classify(const PolyLaunch& a, hipStream_t s);

// Vector layers on a resident image (overlay.hip; dbm_image_overlay): prims (n rows of `stride` float64: xa, ya, xb, yb for segments,
// x, y[, z] for discs) on the device; image uint8 (H, W, channels), painted in place.  overlay_geometry fills the tiling, the radius,
// its square and gmag from H, W, size; overlay_carve hands out overlay_workspace bytes (256-byte aligned; returns the staging area for a
// host table if asked for).  launch_overlay_cull fills conv (the kept primitives in pixel units) and totals = {kept primitives, entries
// the tile bins would hold, primitives with a non-finite coordinate}; the host reads totals, sets kept and -- if it bins -- entries
// (totals[1] indices), then launch_overlay_bin; launch_overlay_paint blends the layer into the image.
struct OverlayLaunch {
  const double* prims;
  long n, H, W;
  int kind, stride, channels, S;     // DBM_OVERLAY_SEGMENTS / _DISCS; doubles per row; 3 or 4; sub-samples per pixel side: 1, 2 or 4
  double x0, y0, dx, dy, size;
  double radius, r2, gmag;           // size / 2, its square as rounded, the largest of W, H and the radius
  long tiles_x, tiles_y, nbins;      // pixel tiles per row, tile rows; tiles_x tiles_y bins
  double* conv;                      // n rows of 4 (segments) or 2 (discs) doubles: the kept primitives, pixel units
  unsigned* cnt;                     // nbins
  unsigned* cursor;                  // nbins
  unsigned* off;                     // nbins + 1
  unsigned* part;                    // per scan tile
  unsigned long long* totals;        // 8
  unsigned* entries;                 // null: unbinned
  unsigned kept;
  unsigned char* image;
  unsigned char rgba[4];
  int word_aligned;                  // the image may be read and written as 32-bit words (channels == 4)
};
void overlay_geometry(OverlayLaunch& a);
size_t overlay_workspace(const OverlayLaunch& a, bool stage_prims_too);
double* overlay_carve(OverlayLaunch& a, void* ws, bool stage_prims_too);
void launch_overlay_cull(const OverlayLaunch& a, hipStream_t s);
void launch_overlay_bin(const OverlayLaunch& a, hipStream_t s);
void launch_overlay_paint(const OverlayLaunch& a, hipStream_t s);
