// Host-side launch sequences of the two deformable layers (final_conv_layer1, 64 -> 64, and final_conv_layer2, 64 -> 1): which kernel
// form runs, in which order, on which scratch.  Generator::forward / backward and the op-level entry points (dbm_op_deform_conv2d*)
// both run these functions; what the two callers own differently -- gradient destinations, prebuilt lists, side streams, a batch of
// weight gradients -- is an argument.  No kernels here.
#include "model.h"

static bool switch_on(const char* name) {   // an A/B switch: on unless set to 0
  const char* v = getenv(name);
  return !(v && atoi(v) == 0);
}

DeformForms deform_layer_forms(int C, int O, int H, int W) {
  // =0: the few-output-channel forward gathers, then multiplies / the 64 -> 1 backward on the gathering kernels / the 64 -> 64 weight
  // gradient from the sample matrix through the 1x1 form.  (A/B switches; every form is parity-tested.)
  static const bool premul = switch_on("DBM_DEFORM1_PREMUL"), premul_bwd = switch_on("DBM_DEFORM1_PREMUL_BWD"),
                    wgrad_fused = switch_on("DBM_DEFORM_WGRAD_FUSED");
  DeformForms f;
  f.fwd_fused = deform_conv_fused_ok(C, O);
  f.fwd_packed = f.fwd_fused ? O == 64 : O != 1;
  f.bwd_fused = f.fwd_fused && deform_input_grad_ok(C, H, W);
  f.premul = f.fwd_fused && O <= 16 && premul;
  f.premul_bwd = f.bwd_fused && O == 1 && premul_bwd;
  f.wgrad_fused = f.bwd_fused && O == 64 && wgrad_fused;
  return f;
}

void deform_layer_forward(const dbm_model& m, const IgLayer* L, const DeformForms& f, const float* x, const float* xt, const float* off,
                          long offsn, const float* w, const float* bias, float* y, float* yt, float* col, float* z, int N, int C, int H,
                          int W, int O, int act, hipStream_t s) {
  DBM_CHECK(!f.fwd_packed || L != nullptr, "deformable layer: this form reads the layer's packed weight image");
  if (f.fwd_fused) {
    launch_deform_conv_fused(xt, off, f.fwd_packed ? L->wf : w, bias, y, yt, col, N, C, H, W, offsn, O, act, 0.2f, s, z);
    return;
  }
  const long P = (long)H * W;
  launch_deform_sample(x, off, col, N, C, H, W, offsn, s);
  if (!f.fwd_packed) {
    launch_gemv_cols(col, w, bias, y, N, C * 9, (int)P, s);
  } else {
    ConvDesc d = m.fwd_desc(*L, col, C * 9 * P, H, W, 0, y, O * P, N);
    d.act = act;
    launch_igemm_conv(d, s);
  }
}

void deform1_backward(const DeformForms& f, const float* x, const float* xt, const float* off, long offsn, const float* w, const float* gy,
                      const float* z, const float* col, float* gx, float* goff, float* gw, float* gb, float* partial, float* csr_ws,
                      float* Gt, bool lists_built, int N, int C, int H, int W, hipStream_t s, hipStream_t s_goff, hipStream_t s_wgrad) {
  const long P = (long)H * W;
  if (f.premul_bwd && z) {
    // Round 5: with z_t = sum_c w[c][t] x_c kept from the forward the layer's whole backward is a CSR gather of ONE value per list entry,
    // four single-float gathers per (position, tap) and one pass over the input -- instead of gathering 9 x 4 x 256 bytes per position
    // for the offset / weight gradients (150 us) and 64 values per entry for the input gradient.
    launch_deform_bwd1_premul(xt, off, w, gy, z, goff, gx, gw, gb, partial, csr_ws, Gt, N, H, W, offsn, s, lists_built);
  } else if (f.bwd_fused) {
    // offset gradients + the layer's weight / bias gradient from one pass over the channels-last input (no sample matrix), next to the
    // input-gradient gather when the caller has a stream for them
    launch_deform_bwd1_fused(xt, off, w, gy, goff, gw, gb, partial, N, H, W, offsn, s_goff);
    launch_deform_input_grad(off, nullptr, w, gy, gx, N, C, H, W, offsn, s, csr_ws, lists_built);
  } else {
    // (the weight gradient only needs gy and the sample matrix: the generator runs it on its side stream, underneath the sampler's backward)
    launch_deform_backward(x, off, nullptr, w, gy, gx, goff, N, C, H, W, offsn, s, csr_ws);
    launch_gemv_cols_wgrad(col, gy, gw, gb, N, C * 9, (int)P, s_wgrad);
  }
}

void deform64_backward_data(const dbm_model& m, const IgLayer& L, const DeformForms& f, const float* x, const float* xt, const float* off,
                            long offsn, const float* gy, float* gcol, float* gx, float* goff, float* csr_ws, bool lists_built, int N, int H,
                            int W, hipStream_t s) {
  const long P = (long)H * W;
  if (f.bwd_fused) {
    // column gradients W^T gy on the MFMAs, offset gradients from the same LDS tile; then the input-gradient gather
    launch_deform_bwd64_fused(xt, off, L.wb[1], gy, gcol, goff, N, H, W, offsn, s);
    launch_deform_input_grad(off, gcol, nullptr, nullptr, gx, N, L.C, H, W, offsn, s, csr_ws, lists_built);
  } else {
    m.run_dgrad(L, dbm_model::dgrad_desc(gy, L.O * P, gcol, L.C * 9 * P, N), H, W, s);
    launch_deform_backward(x, off, gcol, nullptr, nullptr, gx, goff, N, L.C, H, W, offsn, s, csr_ws);
  }
}

void deform64_wgrad(const dbm_model& m, const IgLayer& L, const DeformForms& f, const float* xt, const float* col, const float* off, long offsn,
                    const float* gy, float* gw, float* gb, float* partial, int N, int H, int W, hipStream_t s, WgradBatch* batch) {
  const long P = (long)H * W;
  if (f.wgrad_fused) {
    launch_deform_wgrad64_fused(xt, off, gy, gw, gb, partial, N, H, W, offsn, s);
    return;
  }
  WgradDesc wd = m.wgrad_desc(L, col, L.C * 9 * P, H, W, 0, gy, L.O * P, H, W, N, 1.f);
  wd.gW = gw; wd.gb = gb;
  if (batch) batch->add(wd);
  else launch_wgrad(wd, s);
}
