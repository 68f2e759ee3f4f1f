"""-m gpu: the GEMM-shaped convolution launches (igemm.hip, conv_tile.hip, wgrad.hip) as the MODELS make them -- every epilogue
field in the models' combinations, on strided operands, and weight gradients as batches -- against the float64 NumPy oracle.

dbm_op_conv2d_launch runs one forward / data-gradient launch through fwd_desc / run_dgrad and reports what launch_igemm_conv chose;
dbm_op_conv2d_wgrad_batch runs L descriptors as ONE WgradBatch and reports each descriptor's category and K slices.  Every row of
the tables below names the form it is meant to reach, and the report is asserted: a threshold that moves takes a row's coverage
away loudly.

The epilogue, restated once (`epilogue`):  v = (acc * ch_scale + bias) * s1 + r1s * r1 [c < r1_nch];  if r2: v = s2 * v + r2;
if accumulate: v += y0;  if act: v = lrelu(v);  if mask: v *= lrelu'(mask) [c >= mask_c0]  (both zeros: derivative 1).

What is compared.  EVERY element, against its own float64 L1 mass, so that a wrong tap at a quiet position is not hidden behind the
tensor's maximum: an output element against ((conv(|x|, |w|) * |ch_scale| + |bias|) * |s1| + |r1s * r1|) * |s2| + |r2| + |y0|, a
gW / gb entry against |scale| * sum |dy * x| / |scale| * sum |dy| (plus the prefill's magnitude when it adds onto one: the prefill is
then a term of the sum; an entry whose every term lies outside the image has no mass and must be exactly the prefill).  LeakyReLU is 1-Lipschitz: no exclusions.  Memory a launch must
not touch -- the other channels of a 192-channel concat buffer, channels >= Cout of a padded output, a channels-last twin an igemm
row was offered -- is prefilled with NaN and compared bitwise; operands' channels a launch must not READ (r1 past r1_nch, x past
Cin) hold NaN, mask channels below mask_c0 hold -1.

Tolerance, not taken from the kernels: per quantity (y, gx, gW, gb) 16 x the worst deviation of the FLOAT32 oracle from the float64
one over the whole table in the same normalisation (the kernels' summation depth against NumPy's pairwise / BLAS order, as derived
in test_gpu_norm_ops.py), floor 8 * 2^-24, cap 1e-4; computed at run time (`conv_tolerances`, `wgrad_tolerances`).

Impossible (form x epilogue set) pairs, and why:
  conv_tile x (c)            set (c) is the 9 x 9 trunk's data gradient; conv_tile serves 18- and 36-wide outputs (9-wide only as the
                             OUTPUT of a 4x4 stride-2 FORWARD)
  conv_tile x yt x extras    conv_tile_plan refuses yt with r1 / r2 / accumulate / mask (the twin is written by the plain instance)
  conv_tile cfg 5 / 6 x (b), (c), (g)   data-gradient sets; a 4x4 stride-2 layer's data gradient is the four-phase launch (never conv_tile)
  igemm_pm<16> x data-gradient sets     the same: T = 16 exists only forward
  igemm_pm x (a), (c), (f)   192-channel concat buffers are 9 x 9 trunk planes; igemm_pm takes planes <= 4 x 4
  any data gradient x (d), (e)          run_dgrad sets no bias; ch_scale and yt are forward fields
  igemm x yt                 only conv_tile writes the twin: the op (like Generator::forward) withdraws it, asserted on an igemm row

Found by the bitwise-repeat assertion of row "shared-cat3" (cleared_target 0 and 1, deterministic mode): two descriptors of one
batch that add into the same gW in a pair-buffer category each had a fold job of their own, and the two jobs added their sums a
and b to the gradient g with atomics -- (g + a) + b or (g + b) + a, the same bits only for g = 0 (what the discriminator step
happens to guarantee); under cleared_target both descriptors' first slice pairs went straight to the gradient, four atomic
contributions.  Now such descriptors all go through pair buffers (never pair_direct, also with one slice) and the first one's
fold job adds every member's buffer sum and updates the gradient once: g + (a + b) (WgradPlan::pair_next).  For g = 0 the bits
are the previous ones.

Figures of the run on an MI355X (gfx950) that accompanied this file; the tolerances are computed at run time, these are theirs:
  quantity   float32 oracle's worst   tolerance   kernels' worst
  y               2.42e-07            3.87e-06       3.0e-07
  gx              1.96e-07            3.14e-06       2.7e-07
  gW              2.96e-07            4.73e-06       2.8e-07
  gb              1.32e-07            2.11e-06       5.6e-08
No form needs more than the 16 x margin: the worst kernel figure is 1.4 x the float32 oracle's own.
Kernels' worst |d| / mass per form (rows):
  conv_tile cfg 1                          2.7e-07   ct1-yt ct1-g ct1-gb ct1-a ct1-f
  conv_tile cfg 2                          3.0e-07   ct2-d
  conv_tile cfg 3                          2.4e-07   ct3-d ct3-b ct3-yt
  conv_tile cfg 4                          2.5e-07   ct4-ups ct4-off
  conv_tile cfg 5                          2.5e-07   ct5-yt ct5-d
  conv_tile cfg 6                          2.0e-07   ct6-d
  igemm_pm<9> one tile                     6.0e-08   pm9-1
  igemm_pm<9> two tiles, ksplit 8 / 4      3.3e-08   pm9-2ks pm9-b
  igemm_pm<16> one tile, ksplit 4          2.8e-08   pm16-1ks
  igemm_pm<16> two tiles                   6.7e-08   pm16-2
  igemm_conv W16 NPB 6 ROW                 8.0e-08   ig-w16-f ig-c1 ig-c2-160 ig-c3 ig-odd
  igemm_conv W8 NPB 6 ROW                  5.9e-08   ig-w8-f
  igemm_conv W4 NPB 0 ROW                  7.8e-08   ig-c2-w4
  igemm_conv W4 NPB 0 ROW ksplit 4         7.3e-08   ig-ks-a ig-c1-ks
  igemm_conv W4 NPB -4 ROW (two tiles)     1.1e-07   ig-mt2
  igemm_conv W4 NPB -4 ROW ksplit 4        3.4e-08   ig-mt2-ks
  igemm_conv W16 NPB 6, not ROW (ups)      4.5e-08   ig-ups
  igemm_conv W16 NPB 0, T = 1              5.1e-08   ig-t1
  igemm_conv W4 NPB 0, T = 16, ksplit 4    3.0e-08   ig-t16-ks
  igemm_conv W16 NPB -1 (tap-skip)         4.2e-08   ig-skip
  igemm_conv W4 NPB -1 ksplit 4            2.1e-08   ig-skip-ks
  four phases: W4 ksplit 4 / W16 NPB 6 / W4 NPB -1 ksplit 8     3.9e-08 / 8.3e-08 / 3.8e-08   ig-ph-odd ig-ph-even ig-ph-skip
  one launch per phase (W16 NPB 6)         4.8e-08   ig-ph-1px
  weight gradients, worst over cleared_target x mode, gW / gb:  cat0 2.8e-07 / 5.3e-08, cat1 2.3e-07 / 3.2e-08, cat2 2.8e-07 / 5.3e-08,
    cat3-n5 1.1e-07 / 4.4e-08, cat3-n9 2.1e-07 / 3.3e-08, cat4 2.3e-07 / 5.6e-08, cat5 1.6e-07 / 4.9e-08, cat6 8.1e-08 / 2.6e-08,
    cat7 1.1e-07 / 2.8e-08, cat8 9.0e-08 / 2.5e-08, cat9 1.5e-07 / 2.7e-08, mixed 2.6e-07 / 5.4e-08, tiny-shared 2.2e-07 / -,
    shared-cat3 1.2e-07 / 2.9e-08, fallback 2.4e-07 / 3.5e-08
The module takes 4 s there (149 cases; the slowest, 0.6 s, is the first one, which loads the library).
Mutations tried on a scratch copy (each failed the cases named; test_conv2d_forward / test_conv2d_backward of test_gpu_ops.py passed
all three): `c <= d.r1_nch` in igemm_epilogue_load -> ig-c1 (NaN: r1's channel 64); conv_tile.hip's dnm from d.r1sn -> ct3-b (0.51 of
the mass); `starts[mid] < wg` in wgrad_wave_dma_kernel's plan search -> cat3-n5, cat3-n9, shared-cat3 (0.15 .. 0.85 of the mass; run in
the non-deterministic mode only, where the misdirected workgroup's target is the gradient itself).
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import ops

pytestmark = pytest.mark.gpu

TOL_CAP = 1e-4            # the project's criterion for every dbm_op_* contraction (tests/test_gpu_ops.py)
EPS24 = 2.0 ** -24
TOL_FLOOR = 8 * EPS24
MARGIN = 16.0
RS = 0.2                  # the residual scaling of the dense blocks


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    ctx = _lib.default_context()
    return d, _lib, ctx


def up32(v):
    return (v + 31) // 32 * 32


def cdiv_out(size, k, s, p):
    """floor((size + 2p - k) / s) + 1 with C's truncation: a plane one pixel wide under a 4x4 window still has one output"""
    return int((size + 2 * p - k) / s) + 1


# ------------------------------------------------------------------------------------------------------------------------
# forward / data gradient: the table
# ------------------------------------------------------------------------------------------------------------------------
IG, PM, CT = 0, 1, 2      # report family: igemm_conv_kernel, igemm_pm_kernel, conv_tile_kernel
FIELDS = ("family", "cfg", "waves", "npb", "row", "ksplit", "nosplit", "nphase", "mt2", "yt")


def rep(family, cfg=0, waves=4, npb=0, row=0, ksplit=1, nphase=1, mt2=0, yt=0):
    return (family, cfg, waves, npb, row, ksplit, 0, nphase, mt2, yt)


# id, direction ("F" forward, "D" data gradient), (N, C, H, W, O, k, stride, pad, ups) of the LAYER, epilogue set, options, the
# expected report(s), why.  Epilogue sets (`layout`):
#   plain  bias (forward) only                       a   s1 = rs, r1 (r1_nch = 64), r2, s2 = rs on 192-stride buffers (dense-block tail)
#   b      accumulate + mask, mask_c0 = 0            m   mask alone (the discriminator's conv_layer1 gradient)
#   c1     Cout = 192 gradient: s1, r1 (64 of 192), mask_c0 = 160             c2  accumulate into channels [0, lo) of the buffer whose
#   c3     c2 at lo = 64 with r1, r2 and mask_c0 = 0 (first block of the chain)    slice [lo, lo + 32) is dy, mask_c0 = lo - 32
#   d      ch_scale + bias + act                     e   bias + act + yt (channels-last twin)
#   f      x = first C channels of a 192-channel buffer, y = channels [C, C + 32) of its twin, bias + act
#   g      forward: O = 18 into a 32-channel buffer; data gradient: dy has 32 channel planes (14 of zeros): cin_live, with set b
CONV_ROWS = [
    # ---- conv_tile.hip ----
    ("ct1-yt", "F", (2, 64, 36, 36, 64, 3, 1, 1, 0), "e", {}, [rep(CT, 1, yt=1)], "36-wide rows, 16-byte pieces; plain instance + twin"),
    ("ct1-g", "F", (1, 64, 36, 36, 18, 3, 1, 1, 0), "g", {}, [rep(CT, 1)], "offset conv: 18 of 32 output channels stored"),
    ("ct1-gb", "D", (2, 64, 36, 36, 18, 3, 1, 1, 0), "g", {}, [rep(CT, 1)], "its gradient: cin_live = 24, accumulate + mask (extra instance)"),
    ("ct1-a", "F", (1, 32, 36, 36, 96, 3, 1, 1, 0), "a", {}, [rep(CT, 1)], "extra instance: r1_nch = 64 < Cout = 96, r2, own image strides"),
    ("ct1-f", "F", (1, 96, 36, 36, 32, 3, 1, 1, 0), "f", {}, [rep(CT, 1)], "xsn = ysn = 192 * hw, output slice between canaries"),
    ("ct2-d", "F", (64, 64, 18, 18, 128, 3, 1, 1, 0), "d", {}, [rep(CT, 2)], "N * ceil(Cout / 32) = 256: whole-image workgroups"),
    ("ct3-d", "F", (2, 96, 18, 18, 64, 3, 1, 1, 0), "d", {}, [rep(CT, 3)], "two bands per image, twelve chunks"),
    ("ct3-b", "D", (3, 64, 18, 18, 32, 3, 1, 1, 0), "b", {}, [rep(CT, 3)], "a 3x3 gradient on 18 x 18: reversed tap order through tmap"),
    ("ct3-yt", "F", (3, 32, 18, 18, 64, 3, 1, 1, 0), "e", {}, [rep(CT, 3, yt=1)], "twin from the two-band form"),
    ("ct4-ups", "F", (1, 64, 18, 18, 64, 3, 1, 1, 1), "e", {}, [rep(CT, 4, yt=1)], "post_upsample_2: folded x2 resize -> dword pieces"),
    ("ct4-off", "F", (1, 32, 36, 36, 32, 3, 1, 1, 0), "d", {"xoff": 1}, [rep(CT, 4)], "x one float off 16-byte alignment -> dword pieces"),
    ("ct5-yt", "F", (2, 32, 36, 36, 64, 4, 2, 1, 0), "e", {}, [rep(CT, 5, yt=1)], "4x4 stride 2, 36 -> 18"),
    ("ct5-d", "F", (1, 64, 36, 36, 32, 4, 2, 1, 0), "d", {}, [rep(CT, 5)], "... with the eval-mode BatchNorm fold"),
    ("ct6-d", "F", (3, 32, 18, 18, 64, 4, 2, 1, 0), "d", {}, [rep(CT, 6)], "4x4 stride 2, 18 -> 9: whole image, three tiles"),
    # ---- igemm_pm_kernel ----
    ("pm9-1", "F", (16, 32, 2, 2, 32, 3, 1, 1, 0), "d", {}, [rep(PM)], "<9>, one tile, 32 channels: no K split possible"),
    ("pm9-2ks", "F", (16, 256, 2, 2, 64, 3, 1, 1, 0), "d", {}, [rep(PM, ksplit=8, mt2=1)], "<9>, two tiles, ksplit 8: the last arriver's epilogue"),
    ("pm9-b", "D", (17, 64, 2, 2, 128, 3, 1, 1, 0), "b", {}, [rep(PM, ksplit=4, mt2=1)], "<9> as a data gradient: accumulate + mask behind the fold"),
    ("pm16-1ks", "F", (33, 128, 4, 4, 32, 4, 2, 1, 0), "d", {}, [rep(PM, ksplit=4)], "<16>, one tile, ragged second image group, ksplit 4"),
    ("pm16-2", "F", (16, 32, 4, 4, 64, 4, 2, 1, 0), "d", {}, [rep(PM, mt2=1)], "<16>, two tiles, no split"),
    # ---- igemm_conv_kernel ----
    ("ig-w16-f", "F", (3, 64, 9, 9, 32, 3, 1, 1, 0), "f", {}, [rep(IG, waves=16, npb=6, row=1)], "RDB conv_layer1: 16 wavefronts, register variant, ROW"),
    ("ig-w8-f", "F", (39, 96, 9, 9, 32, 3, 1, 1, 0), "f", {}, [rep(IG, waves=8, npb=6, row=1)], "> 96 tiles, 96 channels: 8 wavefronts; ragged last tile"),
    ("ig-ks-a", "F", (2, 192, 9, 9, 64, 3, 1, 1, 0), "a", {}, [rep(IG, waves=4, row=1, ksplit=4)], "RDB conv_layer5: ksplit 4 with r1 + r2 loaded by the last arriver"),
    ("ig-c1", "D", (2, 192, 9, 9, 64, 3, 1, 1, 0), "c1", {}, [rep(IG, waves=16, npb=6, row=1)], "its gradient: Cout 192, r1_nch 64, mask_c0 160"),
    ("ig-c1-ks", "D", (2, 192, 9, 9, 128, 3, 1, 1, 0), "c1", {}, [rep(IG, waves=4, row=1, ksplit=4)], "the same set behind a K split: r1_nch 64 of 192 and mask_c0 160 loaded by the last arriver"),
    ("ig-c2-w4", "D", (13, 96, 9, 9, 32, 3, 1, 1, 0), "c2", {}, [rep(IG, waves=4, row=1)], "short K (32): 4 wavefronts, streaming; accumulate at ysn = 192 * 81, mask_c0 = 64"),
    ("ig-c2-160", "D", (5, 160, 9, 9, 32, 3, 1, 1, 0), "c2", {}, [rep(IG, waves=16, npb=6, row=1)], "lo = 160: mask_c0 = 128, no canary channels left"),
    ("ig-c3", "D", (3, 64, 9, 9, 32, 3, 1, 1, 0), "c3", {}, [rep(IG, waves=16, npb=6, row=1)], "first block of the chain: accumulate + r1 + r2 + mask_c0 0"),
    ("ig-mt2-ks", "F", (13, 128, 9, 9, 64, 3, 1, 1, 0), "d", {"yt": 1}, [rep(IG, waves=4, npb=-4, row=1, ksplit=4, mt2=1)], "two tiles per wavefront + ksplit 4; offered a twin: untouched"),
    ("ig-mt2", "F", (52, 128, 9, 9, 64, 3, 1, 1, 0), "d", {}, [rep(IG, waves=4, npb=-4, row=1, mt2=1)], "two tiles, 132 workgroups: no split"),
    ("ig-ups", "F", (2, 64, 5, 5, 64, 3, 1, 1, 1), "plain", {"act": 1}, [rep(IG, waves=16, npb=6)], "folded resize on a 10 x 10 output: not ROW"),
    ("ig-odd", "F", (1, 64, 13, 17, 32, 3, 1, 1, 0), "b", {}, [rep(IG, waves=16, npb=6, row=1)], "odd non-square plane"),
    ("ig-t1", "F", (2, 576, 6, 6, 64, 1, 1, 0, 0), "d", {}, [rep(IG, waves=16)], "T = 1 (the deformable layer's GEMM), 18 channel pairs: streaming"),
    ("ig-t16-ks", "F", (3, 128, 9, 9, 256, 4, 2, 1, 0), "d", {}, [rep(IG, waves=4, ksplit=4)], "D conv_layer5, 9 -> 4 (odd input), T = 16, ksplit 4"),
    ("ig-skip", "F", (3, 32, 2, 2, 32, 4, 2, 1, 0), "d", {}, [rep(IG, waves=16, npb=-1)], "N < 16 on a 2 x 2 plane: tap-skip, one workgroup per tile"),
    ("ig-skip-ks", "F", (5, 128, 2, 2, 64, 4, 2, 1, 0), "d", {}, [rep(IG, waves=4, npb=-1, ksplit=4)], "... with ksplit 4"),
    ("ig-ph-odd", "D", (3, 128, 9, 9, 256, 4, 2, 1, 0), "plain", {}, [rep(IG, waves=4, ksplit=4, nphase=4)], "four phases, 9 <- 4: planes 5x5 5x4 4x5 4x4, ksplit 4"),
    ("ig-ph-even", "D", (1, 32, 36, 36, 32, 4, 2, 1, 0), "m", {}, [rep(IG, waves=16, npb=6, nphase=4)], "four phases, 36 <- 18, mask alone (D conv_layer1)"),
    ("ig-ph-skip", "D", (3, 64, 4, 4, 256, 4, 2, 1, 0), "plain", {}, [rep(IG, waves=4, npb=-1, ksplit=8, nphase=4)], "four phases of a 2 x 2 gradient: T = 4 tap-skip, ksplit 8"),
    ("ig-ph-1px", "D", (2, 32, 6, 1, 32, 4, 2, 1, 0), "b", {}, [rep(IG, waves=16, npb=6), rep(IG, waves=16, npb=6)], "a plane one pixel wide: one launch per existing phase (px = 1 has none)"),
]
CONV_IDS = [r[0] for r in CONV_ROWS]


def lrelu_mask(rs, shape):
    """|m| >= 0.1 with random signs, plus a handful of exact +0.0 and -0.0 entries (both: derivative 1)"""
    m = (rs.uniform(0.1, 2.0, size=shape) * rs.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    flat = m.reshape(-1)
    idx = rs.choice(flat.size, size=min(8, flat.size), replace=False)
    flat[idx[0::2]] = 0.0
    flat[idx[1::2]] = -0.0
    return m


def epilogue(acc, t, dtype):
    """THE formula (module docstring) in `dtype`; t: bias, chs, s1, r1, r1_nch, r1s, r2, s2, y0, act, mask, mask_c0"""
    f = np.dtype(dtype).type
    v = acc.astype(dtype, copy=True)
    if t.get("chs") is not None:
        v = v * t["chs"].astype(dtype)[None, :, None, None]
    if t.get("bias") is not None:
        v = v + t["bias"].astype(dtype)[None, :, None, None]
    v = v * f(t.get("s1", 1.0))
    if t.get("r1") is not None:
        v[:, :t["r1_nch"]] += f(t["r1s"]) * t["r1"].astype(dtype)
    if t.get("r2") is not None:
        v = f(t["s2"]) * v + t["r2"].astype(dtype)
    if t.get("y0") is not None:
        v = v + t["y0"].astype(dtype)
    if t.get("act"):
        v = ops.leaky_relu(v)
    if t.get("mask") is not None:
        c0 = t["mask_c0"]
        v[:, c0:] = ops.leaky_relu_backward(t["mask"][:, c0:].astype(dtype), v[:, c0:])
    return v


def conv_acc(direction, shape, x, w, dtype):
    """The convolution sum of the launch in `dtype`: forward conv of the (resized) input, or the oracle's data gradient"""
    N, Cc, H, W, O, k, s, p, ups = shape
    x, w = x.astype(dtype), w.astype(dtype)
    if direction == "F":
        return ops.conv2d(ops.upsample_nearest2(x) if ups else x, w, None, s, p)
    # (a plane narrower than the window: the same sums on the plane widened with zero columns / rows)
    He, We = max(H, k - 2 * p), max(W, k - 2 * p)
    wp = np.zeros((x.shape[1], Cc, k, k), dtype)
    wp[:O] = w
    gx, _, _ = ops.conv2d_backward(np.zeros((N, Cc, He, We), dtype), wp, x, s, p)
    return np.ascontiguousarray(gx[:, :, :H, :W])


def layout(row):
    """Host buffers of a row: name -> float32 array (N, channels, h, w) as uploaded, operand views into them, epilogue tensors"""
    rid, direction, shape, epi, opt, _, _ = row
    N, Cc, H, W, O, k, s, p, ups = shape
    rs = np.random.RandomState([zlib.crc32(rid.encode()), N, Cc, H, W, O])   # (independent of the row's place in the table)
    OH, OW = cdiv_out(H << ups, k, s, p), cdiv_out(W << ups, k, s, p)
    if direction == "F":
        xc, xh, xw, oc, oh, ow = Cc, H, W, O, OH, OW
    else:
        xc, xh, xw, oc, oh, ow = up32(O), OH, OW, Cc, H, W
    nan = np.float32(np.nan)
    w = (rs.normal(size=(O, Cc, k, k)) / np.sqrt(Cc * k * k)).astype(np.float32)
    x = rs.normal(size=(N, xc, xh, xw)).astype(np.float32)
    if direction == "D" and O < xc:
        x[:, O:] = 0.0   # (padded gradient channels: zeros, as the models keep them)
    B, t = {}, {"act": opt.get("act", 0), "s1": 1.0, "r1s": 1.0, "s2": 1.0}
    A = {}   # operand -> (buffer name, first channel)

    def buf(name, channels, h, w_, fill=nan):
        B[name] = np.full((N, channels, h, w_), fill, np.float32)
        return B[name]

    def place(name, data, channels=None, c0=0, fill=nan):
        b = buf(name, channels or data.shape[1], data.shape[2], data.shape[3], fill)
        b[:, c0:c0 + data.shape[1]] = data
        return b

    # x and y
    if epi == "c2" or epi == "c3":
        lo = Cc
        D = buf("y", 192, oh, ow)
        D[:, lo:lo + 32] = x
        t["y0"] = rs.normal(size=(N, oc, oh, ow)).astype(np.float32)
        D[:, :lo] = t["y0"]
        A["x"], A["y"] = ("y", lo), ("y", 0)
    else:
        xch = 192 if epi in ("a", "f") else xc
        place("x", x, xch)
        A["x"] = ("x", 0)
        ych, yc0 = (192, 0) if epi in ("a", "c1") else (192, Cc) if epi == "f" else (32, 0) if (epi == "g" and direction == "F") else (oc, 0)
        buf("y", ych, oh, ow)
        A["y"] = ("y", yc0)
        if epi in ("b",) or (epi == "g" and direction == "D"):
            t["y0"] = rs.normal(size=(N, oc, oh, ow)).astype(np.float32)
            B["y"][:, yc0:yc0 + oc] = t["y0"]
    if direction == "F" and epi != "c1":
        t["bias"] = rs.normal(size=O).astype(np.float32)
    if epi == "d":
        t["chs"] = (rs.uniform(0.5, 1.5, O) * rs.choice([-1.0, 1.0], O)).astype(np.float32)
        t["act"] = 1
    if epi in ("e", "f"):
        t["act"] = 1
    if epi == "a":
        t["s1"], t["s2"], t["r1_nch"] = RS, RS, 64
        t["r1"] = rs.normal(size=(N, 64, oh, ow)).astype(np.float32)
        t["r2"] = rs.normal(size=(N, oc, oh, ow)).astype(np.float32)
        place("r1", t["r1"], 192)
        place("r2", t["r2"], 192)
        A["r1"], A["r2"] = ("r1", 0), ("r2", 0)
    if epi == "c1":
        t["s1"], t["r1s"], t["r1_nch"], t["mask_c0"] = RS * RS, RS, 64, 160
        t["r1"] = rs.normal(size=(N, 64, oh, ow)).astype(np.float32)
        place("r1", t["r1"], 96)
        A["r1"] = ("r1", 0)
    if epi == "c3":
        t["r1_nch"] = 64
        t["r1"] = rs.normal(size=(N, 64, oh, ow)).astype(np.float32)
        t["r2"] = rs.normal(size=(N, 64, oh, ow)).astype(np.float32)
        place("r1", t["r1"], 192)
        place("r2", t["r2"], 64)
        A["r1"], A["r2"] = ("r1", 0), ("r2", 0)
        t["mask_c0"] = 0
    if epi == "c2":
        t["mask_c0"] = Cc - 32
    if epi in ("b", "m") or (epi == "g" and direction == "D"):
        t["mask_c0"] = 0
    if "mask_c0" in t:
        mch = 192 if epi in ("c1", "c2", "c3") else oc
        m = buf("mask", mch, oh, ow, np.float32(-1.0))   # (channels a launch must not read: a wrong read scales by 0.2)
        m[:, :oc] = lrelu_mask(rs, (N, oc, oh, ow))
        t["mask"] = m[:, :oc].copy()
        m[:, :t["mask_c0"]] = -1.0
        A["mask"] = ("mask", 0)
    want_yt = epi == "e" or opt.get("yt")
    if want_yt:
        B["yt"] = np.full((N * oh * ow, 64), nan, np.float32)
    return dict(B=B, A=A, t=t, w=w, x=x, dims=(xc, xh, xw, oc, oh, ow), xoff=opt.get("xoff", 0), want_yt=bool(want_yt))


@functools.lru_cache(maxsize=None)
def conv_case(rid):
    """Inputs of a row, its float64 reference and L1 mass, and the float32 oracle's deviation; shared, never modified"""
    row = CONV_ROWS[CONV_IDS.index(rid)]
    _, direction, shape, _, _, _, _ = row
    L = layout(row)
    t = L["t"]
    ref = epilogue(conv_acc(direction, shape, L["x"], L["w"], np.float64), t, np.float64)
    ab = {k_: (np.abs(v) if isinstance(v, np.ndarray) else abs(v) if isinstance(v, float) else v) for k_, v in t.items()}
    ab.update(act=0, mask=None)
    mass = epilogue(conv_acc(direction, shape, np.abs(L["x"]), np.abs(L["w"]), np.float64), ab, np.float64)
    r32 = epilogue(conv_acc(direction, shape, L["x"], L["w"], np.float32), t, np.float32)
    L.update(ref=ref, mass=mass, dev32=rel_mass(r32.astype(np.float64) - ref, mass))
    return L


def rel_mass(diff, mass):
    """max |diff| / mass; an entry without mass (every term it sums lies outside the image) must be exact"""
    diff, mass = np.abs(np.asarray(diff, np.float64)), np.asarray(mass, np.float64)
    r = np.where(mass > 0, diff / np.where(mass > 0, mass, 1.0), np.where(diff == 0, 0.0, np.inf))
    return float(r.max())


def tolerance(worst32):
    return float(min(max(MARGIN * worst32, TOL_FLOOR), TOL_CAP))


@functools.lru_cache(maxsize=None)
def conv_tolerances():
    """{'y': ..., 'gx': ...}: 16 x the float32 oracle's worst deviation over the whole table, floor 8 * 2^-24, cap 1e-4"""
    worst = {"F": 0.0, "D": 0.0}
    for row in CONV_ROWS:
        worst[row[1]] = max(worst[row[1]], conv_case(row[0])["dev32"])
    return {"y": tolerance(worst["F"]), "gx": tolerance(worst["D"]), "worst32": worst}


def run_conv(dbm, rid):
    """One call of dbm_op_conv2d_launch on fresh device buffers: (y buffer after, yt after or None, reports)"""
    d, _lib, ctx = dbm
    row = CONV_ROWS[CONV_IDS.index(rid)]
    _, direction, shape, _, _, _, _ = row
    N, Cc, H, W, O, k, s, p, ups = shape
    L = conv_case(rid)
    dev, ptr = {}, {}
    for name, host in L["B"].items():
        if name == "x" and L["xoff"]:
            flat = np.concatenate([np.zeros(L["xoff"], np.float32), host.reshape(-1)])
            dev[name] = d.to_device(flat)
            ptr[name] = dev[name].ptr + 4 * L["xoff"]
        else:
            dev[name] = d.to_device(host)
            ptr[name] = dev[name].ptr
    t = L["t"]
    small = {n_: d.to_device(v) for n_, v in (("w", L["w"]), ("bias", t.get("bias")), ("chs", t.get("chs"))) if v is not None}

    def operand(name):
        if name not in L["A"]:
            return None, 0
        b, c0 = L["A"][name]
        plane = L["B"][b].shape[2] * L["B"][b].shape[3]
        return ptr[b] + 4 * c0 * plane, L["B"][b].shape[1] * plane

    a = _lib.ConvLaunch()
    a.dgrad = int(direction == "D")
    a.N, a.C, a.H, a.W, a.O, a.k, a.stride, a.pad, a.ups = N, Cc, H, W, O, k, s, p, ups
    a.w = small["w"].ptr
    a.bias = small["bias"].ptr if "bias" in small else None
    a.x, a.xsn = operand("x")
    a.y, a.ysn = operand("y")
    a.act, a.s1, a.r1s, a.s2 = int(t["act"]), t["s1"], t["r1s"], t["s2"]
    a.r1, a.r1sn = operand("r1")
    a.r1_nch = t.get("r1_nch", 0)
    a.r2, a.r2sn = operand("r2")
    a.accumulate = int(t.get("y0") is not None)
    a.mask, a.masksn = operand("mask")
    a.mask_c0 = t.get("mask_c0", 0)
    a.ch_scale = small["chs"].ptr if "chs" in small else None
    a.yt = dev["yt"].ptr if L["want_yt"] else None
    report = (C.c_int * _lib.CONV_REPORT_INTS)()
    _lib.check(_lib.lib().dbm_op_conv2d_launch(ctx.handle, C.byref(a), report), ctx.handle)
    reps = [tuple(report[1 + 10 * i:11 + 10 * i]) for i in range(report[0])]
    return dev["y"].get(), (dev["yt"].get() if L["want_yt"] else None), reps


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def conv_error(rid, ybuf):
    """(worst |d| / mass over the written region, whether everything else kept its prefill bit for bit)"""
    L = conv_case(rid)
    _, c0 = L["A"]["y"]
    oc = L["dims"][3]
    got = ybuf[:, c0:c0 + oc].astype(np.float64)
    err = rel_mass(got - L["ref"], L["mass"]) if np.isfinite(got).all() else float("inf")
    keep = np.ones(ybuf.shape[1], bool)
    keep[c0:c0 + oc] = False
    untouched = np.array_equal(bits(ybuf[:, keep]), bits(L["B"]["y"][:, keep]))
    return err, untouched


@pytest.mark.parametrize("rid", CONV_IDS)
def test_conv_launch(dbm, rid):
    row = CONV_ROWS[CONV_IDS.index(rid)]
    _, direction, shape, epi, opt, expect, why = row
    L = conv_case(rid)
    tol = conv_tolerances()["y" if direction == "F" else "gx"]
    ybuf, yt, reps = run_conv(dbm, rid)
    err, untouched = conv_error(rid, ybuf)
    print(f"{rid}: {dict(zip(FIELDS, reps[0]))} x{len(reps)}  err/mass {err:.3e}  float32 oracle {L['dev32']:.3e}  tol {tol:.3e}")
    assert reps == expect, (why, [dict(zip(FIELDS, r)) for r in reps])
    assert untouched, "the launch wrote outside its output channels"
    assert err <= tol, (err, tol)
    if L["want_yt"]:
        if expect[0][FIELDS.index("yt")]:
            _, c0 = L["A"]["y"]
            nhwc = np.ascontiguousarray(ybuf[:, c0:c0 + 64].transpose(0, 2, 3, 1)).reshape(-1, 64)
            assert np.array_equal(bits(yt), bits(nhwc)), "the channels-last twin differs from y"
        else:
            assert np.isnan(yt).all() and np.array_equal(bits(yt), bits(L["B"]["yt"])), "an igemm launch touched yt"
    if expect[0][0] == CT or any(r[FIELDS.index("ksplit")] > 1 for r in expect):
        # no split-K, resp. a fold that claims independence of arrival order: the same bits every time
        ybuf2, yt2, reps2 = run_conv(dbm, rid)
        assert reps2 == reps
        assert np.array_equal(bits(ybuf2), bits(ybuf))
        if yt is not None:
            assert np.array_equal(bits(yt2), bits(yt))


def test_ksplit_arrival_counters_are_back_at_zero(dbm):
    """Split-K launches of different tile counts and splits back to back on one stream share the arrival counters: each last arriver
    leaves its counter at zero, else the next launch's tiles never find their last arriver (their outputs keep the NaN prefill)"""
    order = ["ig-ks-a", "pm9-2ks", "ig-t16-ks", "ig-ph-skip", "pm16-1ks", "ig-c1-ks", "ig-ks-a", "ig-mt2-ks", "pm9-2ks"]
    first = {}
    for rid in order:
        ybuf, _, reps = run_conv(dbm, rid)
        assert reps[0][FIELDS.index("ksplit")] > 1
        err, untouched = conv_error(rid, ybuf)
        row = CONV_ROWS[CONV_IDS.index(rid)]
        assert untouched and err <= conv_tolerances()["y" if row[1] == "F" else "gx"], (rid, err)
        if rid in first:
            assert np.array_equal(bits(ybuf), bits(first[rid])), rid
        first[rid] = ybuf


# ------------------------------------------------------------------------------------------------------------------------
# the forms the comments over CONV_CASES (test_gpu_ops.py) promise, pinned: every hand-picked row with >= 32 input channels
# through the new forward op with a plain epilogue (bias, the row's LeakyReLU)
# ------------------------------------------------------------------------------------------------------------------------
PINNED_FORMS = {
    # (N, C, H, W, O, k, stride, pad, ups, lrelu): report  -- PINNED_BEGIN
    (3, 64, 9, 9, 32, 3, 1, 1, 0, 1): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (2, 192, 9, 9, 64, 3, 1, 1, 0, 0): (0, 0, 4, 0, 1, 4, 0, 1, 0, 0),
    (5, 128, 9, 9, 64, 3, 1, 1, 0, 1): (0, 0, 4, 0, 1, 4, 0, 1, 0, 0),
    (2, 64, 9, 9, 64, 3, 1, 1, 1, 1): (2, 3, 4, 0, 0, 1, 0, 1, 0, 0),
    (1, 64, 18, 18, 64, 3, 1, 1, 1, 1): (2, 4, 4, 0, 0, 1, 0, 1, 0, 0),
    (2, 64, 36, 36, 18, 3, 1, 1, 0, 0): (2, 1, 4, 0, 0, 1, 0, 1, 0, 0),
    (3, 64, 36, 36, 64, 4, 2, 1, 0, 0): (2, 5, 4, 0, 0, 1, 0, 1, 0, 0),
    (3, 128, 9, 9, 256, 4, 2, 1, 0, 0): (0, 0, 4, 0, 0, 4, 0, 1, 0, 0),
    (4, 512, 2, 2, 512, 4, 2, 1, 0, 0): (0, 0, 4, -1, 0, 16, 0, 1, 0, 0),
    (2, 256, 4, 4, 256, 3, 1, 1, 0, 0): (0, 0, 4, 0, 1, 8, 0, 1, 0, 0),
    (1, 64, 13, 17, 32, 3, 1, 1, 0, 1): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (2, 576, 6, 6, 64, 1, 1, 0, 0, 1): (0, 0, 16, 0, 0, 1, 0, 1, 0, 0),
    (67, 96, 9, 9, 32, 3, 1, 1, 0, 1): (0, 0, 8, 6, 1, 1, 0, 1, 0, 0),
    (70, 160, 9, 9, 32, 3, 1, 1, 0, 0): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (64, 32, 9, 9, 64, 3, 1, 1, 0, 0): (0, 0, 4, 0, 1, 1, 0, 1, 0, 0),
    (33, 256, 4, 4, 512, 3, 1, 1, 0, 0): (0, 0, 4, -4, 1, 1, 0, 1, 1, 0),
    (37, 512, 2, 2, 512, 3, 1, 1, 0, 0): (1, 0, 4, 0, 0, 8, 0, 1, 1, 0),
    (9, 64, 18, 18, 128, 3, 1, 1, 0, 0): (2, 3, 4, 0, 0, 1, 0, 1, 0, 0),
    (5, 64, 11, 13, 32, 3, 1, 1, 0, 0): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (24, 64, 36, 36, 64, 3, 1, 1, 0, 0): (2, 1, 4, 0, 0, 1, 0, 1, 0, 0),
    (20, 64, 18, 18, 64, 3, 1, 1, 1, 0): (2, 4, 4, 0, 0, 1, 0, 1, 0, 0),
    (12, 96, 36, 36, 32, 4, 2, 1, 0, 0): (2, 5, 4, 0, 0, 1, 0, 1, 0, 0),
    (3, 64, 23, 21, 32, 3, 1, 1, 0, 0): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (2, 32, 21, 19, 64, 4, 2, 1, 0, 0): (0, 0, 16, 0, 0, 1, 0, 1, 0, 0),
    (9, 576, 36, 36, 64, 1, 1, 0, 0, 0): (0, 0, 8, 0, 0, 1, 0, 1, 0, 0),
    (3, 160, 20, 20, 96, 1, 1, 0, 0, 0): (0, 0, 16, 6, 0, 1, 0, 1, 0, 0),
    (64, 128, 9, 9, 256, 4, 2, 1, 0, 0): (0, 0, 4, -4, 0, 2, 0, 1, 1, 0),
    (37, 256, 4, 4, 512, 4, 2, 1, 0, 0): (1, 0, 4, 0, 0, 8, 0, 1, 1, 0),
    (64, 512, 2, 2, 512, 3, 1, 1, 0, 0): (1, 0, 4, 0, 0, 8, 0, 1, 1, 0),
    (64, 512, 2, 2, 512, 4, 2, 1, 0, 0): (1, 0, 4, 0, 0, 16, 0, 1, 1, 0),
    (64, 256, 4, 4, 512, 4, 2, 1, 0, 1): (1, 0, 4, 0, 0, 8, 0, 1, 1, 0),
    (16, 256, 4, 4, 256, 3, 1, 1, 0, 1): (0, 0, 4, -4, 1, 8, 0, 1, 1, 0),
    (40, 64, 3, 2, 64, 3, 1, 1, 0, 0): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (33, 96, 4, 3, 32, 3, 1, 1, 0, 0): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (48, 128, 1, 1, 96, 3, 1, 1, 0, 0): (1, 0, 4, 0, 0, 4, 0, 1, 0, 0),
    (64, 96, 2, 2, 160, 4, 2, 1, 0, 0): (0, 0, 4, -1, 0, 2, 0, 1, 0, 0),
    (1, 96, 1, 1, 32, 1, 1, 0, 0, 0): (0, 0, 16, 6, 0, 1, 0, 1, 0, 0),
    (3, 96, 2, 1, 32, 1, 1, 0, 0, 0): (0, 0, 16, 6, 0, 1, 0, 1, 0, 0),
    (2, 64, 5, 1, 64, 3, 1, 1, 0, 1): (0, 0, 16, 6, 1, 1, 0, 1, 0, 0),
    (64, 64, 18, 18, 128, 3, 1, 1, 0, 1): (2, 2, 4, 0, 0, 1, 0, 1, 0, 0),
    (3, 96, 18, 18, 64, 3, 1, 1, 0, 0): (2, 3, 4, 0, 0, 1, 0, 1, 0, 0),
    (2, 32, 36, 36, 64, 3, 1, 1, 0, 1): (2, 1, 4, 0, 0, 1, 0, 1, 0, 0),
    (2, 160, 36, 36, 96, 3, 1, 1, 0, 0): (2, 1, 4, 0, 0, 1, 0, 1, 0, 0),
    (3, 128, 9, 9, 64, 3, 1, 1, 1, 1): (2, 3, 4, 0, 0, 1, 0, 1, 0, 0),
    (5, 128, 18, 18, 128, 4, 2, 1, 0, 1): (2, 6, 4, 0, 0, 1, 0, 1, 0, 0),
    (7, 64, 36, 36, 96, 4, 2, 1, 0, 0): (2, 5, 4, 0, 0, 1, 0, 1, 0, 0),
    (64, 128, 9, 9, 128, 3, 1, 1, 0, 1): (0, 0, 4, -4, 1, 1, 0, 1, 1, 0),
    # PINNED_END
}


def _hand_picked():
    from test_gpu_ops import CONV_CASES

    n_random = 14 + 12   # _random_conv_cases(404, 14) + _random_tail_cases(77, 12), appended last
    return [c for c in CONV_CASES[:-n_random] if c[1] % 32 == 0]


HAND_PICKED = _hand_picked()


@pytest.mark.parametrize("case", HAND_PICKED)
def test_conv_cases_reach_the_forms_their_comments_promise(dbm, case):
    d, _lib, ctx = dbm
    N, Cc, H, W, O, k, s, p, ups, act = case
    rs = np.random.RandomState(hash(case) % 2**31)
    x = rs.normal(size=(N, Cc, H, W)).astype(np.float32)
    w = (rs.normal(size=(O, Cc, k, k)) / np.sqrt(Cc * k * k)).astype(np.float32)
    b = rs.normal(size=(O,)).astype(np.float32)
    OH, OW = cdiv_out(H << ups, k, s, p), cdiv_out(W << ups, k, s, p)
    dx, dw, db = d.to_device(x), d.to_device(w), d.to_device(b)
    y = d.to_device(np.full((N, O, OH, OW), np.nan, np.float32))
    a = _lib.ConvLaunch()
    a.N, a.C, a.H, a.W, a.O, a.k, a.stride, a.pad, a.ups = N, Cc, H, W, O, k, s, p, ups
    a.w, a.bias, a.x, a.xsn, a.y, a.ysn = dw.ptr, db.ptr, dx.ptr, Cc * H * W, y.ptr, O * OH * OW
    a.act, a.s1, a.r1s, a.s2 = act, 1.0, 1.0, 1.0
    report = (C.c_int * _lib.CONV_REPORT_INTS)()
    _lib.check(_lib.lib().dbm_op_conv2d_launch(ctx.handle, C.byref(a), report), ctx.handle)
    got = tuple(report[1:11])
    print(f"PIN {case}: {got}")
    assert report[0] == 1
    assert np.isfinite(y.get()).all()
    assert got == PINNED_FORMS[case], dict(zip(FIELDS, got))


# ------------------------------------------------------------------------------------------------------------------------
# batched weight gradients
# ------------------------------------------------------------------------------------------------------------------------
def wd(shape, scale=1.0, gb=True, x=None, dy=None, share=None, xoff=0):
    """One descriptor: (N, C, H, W, O, k, stride, pad, ups); x / dy = (buffer name, channels of the buffer, first channel) to place
    the operand in a shared or wider buffer; share = index of the descriptor whose gW / gb this one adds into"""
    return dict(shape=shape, scale=scale, gb=gb, x=x, dy=dy, share=share, xoff=xoff)


def trunk(N, scale_at):
    """The dense block's pattern: Cin in {64 .. 192} as prefixes of ONE 192-channel buffer, dy = 32-channel slices of another"""
    out = []
    for i, cin in enumerate((64, 96, 128, 160, 192)):
        out.append(wd((N, cin, 9, 9, 32, 3, 1, 1, 0), scale=RS if i == scale_at else 1.0, x=("X", 192, 0), dy=("D", 192, 32 * i)))
    return out


# id, descriptors, expected [(category, S deterministic, S non-deterministic)] per descriptor, special ("fallback": assert only that
# the category is neither 3 nor 9), why
WGRAD_ROWS = [
    ("cat0", [wd((2, 576, 6, 6, 64, 1, 1, 0, 0)), wd((3, 96, 2, 1, 32, 1, 1, 0, 0), gb=False), wd((1, 96, 1, 1, 32, 1, 1, 0, 0))],
     None, None, "1x1 workgroup form: three sizes, gb null in the middle"),
    ("cat1", [wd((2, 64, 3, 3, 64, 3, 1, 1, 1)), wd((2, 64, 5, 1, 64, 3, 1, 1, 0), gb=False), wd((3, 96, 4, 5, 32, 3, 1, 1, 0), xoff=1)],
     None, None, "3x3 workgroup form: a resized 3 x 3 plane, a plane one pixel wide, an x one float off alignment"),
    ("cat2", [wd((5, 64, 11, 9, 32, 4, 2, 1, 0), gb=False), wd((17, 96, 4, 4, 64, 4, 2, 1, 0)), wd((3, 32, 7, 5, 96, 4, 2, 1, 0))],
     None, None, "4x4 workgroup form: a 5 x 4 output (two K slices), then two that only gb non-null keeps off wgrad_s2tiny_kernel"),
    ("cat3-n5", trunk(5, 4), None, None, "trunk pattern, N = 5: strided prefixes / slices, scale 0.2 on conv_layer5, S odd"),
    ("cat3-n9", trunk(9, 0)[:3] + [wd((4, 32, 4, 4, 64, 3, 1, 1, 0)), wd((2, 64, 9, 9, 64, 3, 1, 1, 0), gb=False)], None, None,
     "N = 9 prefixes + a 4 x 4 plane (S even) + N = 2: S = 2, no pair buffer under cleared_target"),
    ("cat4", [wd((5, 64, 11, 13, 32, 3, 1, 1, 0)), wd((2, 32, 5, 5, 64, 3, 1, 1, 1), gb=False), wd((1, 96, 12, 9, 96, 3, 1, 1, 0))],
     None, None, "3x3 row bands: odd plane, resized 5 x 5, three tiles"),
    ("cat5", [wd((2, 32, 21, 19, 64, 4, 2, 1, 0)), wd((3, 64, 18, 18, 32, 4, 2, 1, 0), gb=False), wd((1, 96, 24, 20, 96, 4, 2, 1, 0))],
     None, None, "4x4 row bands: odd input, 18 -> 9, three tiles"),
    ("cat6", [wd((2, 64, 36, 36, 64, 3, 1, 1, 0)), wd((3, 64, 23, 21, 32, 3, 1, 1, 0), gb=False), wd((1, 96, 18, 18, 96, 3, 1, 1, 0))],
     None, None, "direct 3x3: 4.5 segments per row, odd widths, 2.25 segments"),
    ("cat7", [wd((2, 64, 18, 18, 64, 3, 1, 1, 1)), wd((3, 32, 9, 9, 32, 3, 1, 1, 1), gb=False), wd((1, 96, 10, 12, 96, 3, 1, 1, 1))],
     None, None, "direct 3x3 on a resized input"),
    ("cat8", [wd((2, 96, 36, 36, 32, 4, 2, 1, 0)), wd((3, 32, 32, 40, 64, 4, 2, 1, 0), gb=False), wd((1, 64, 36, 36, 96, 4, 2, 1, 0))],
     None, None, "direct 4x4 stride 2: both tap halves"),
    ("cat9", [wd((2, 160, 20, 20, 96, 1, 1, 0, 0)), wd((3, 64, 16, 16, 32, 1, 1, 0, 0), gb=False), wd((1, 576, 18, 18, 64, 1, 1, 0, 0))],
     None, None, "1x1 GEMM on large planes: two output groups, ragged bands and channel groups"),
    ("mixed", [wd((1, 96, 1, 1, 32, 1, 1, 0, 0)), wd((2, 64, 18, 18, 64, 1, 1, 0, 0)), wd((5, 96, 9, 9, 32, 3, 1, 1, 0)),
               wd((1, 64, 36, 36, 32, 3, 1, 1, 0), gb=False), wd((2, 64, 11, 13, 32, 3, 1, 1, 0)), wd((5, 64, 9, 9, 32, 4, 2, 1, 0)),
               wd((16, 64, 4, 4, 32, 4, 2, 1, 0), gb=False)],
     None, None, "1x1 small and large, wave-DMA, direct, row band, 4x4 workgroup form, tiny: every category's launch and fold in one call"),
    ("tiny-shared", [wd((16, 64, 4, 4, 32, 4, 2, 1, 0), gb=False), wd((16, 64, 4, 4, 32, 4, 2, 1, 0), gb=False, share=0),
                     wd((37, 32, 2, 2, 64, 3, 1, 1, 0), gb=False, scale=0.5), wd((37, 32, 2, 2, 64, 3, 1, 1, 0), gb=False, scale=0.5, share=2),
                     wd((21, 32, 4, 4, 32, 3, 1, 1, 0), gb=False)],
     None, None, "wgrad_s2tiny_kernel: real + fake into one gW through a shared plan, K = 4 and K = 3, and a single-graph plan"),
    ("shared-cat3", [wd((5, 64, 9, 9, 32, 3, 1, 1, 0)), wd((5, 64, 9, 9, 32, 3, 1, 1, 0), share=0), wd((3, 96, 9, 9, 64, 3, 1, 1, 0), gb=False)],
     None, None, "two descriptors add into one gW / gb in a non-tiny category"),
    ("fallback", [wd((5, 64, 9, 9, 32, 3, 1, 1, 0), xoff=1), wd((3, 64, 5, 5, 32, 3, 1, 1, 0), dy=("D33", 33, 0)),
                  wd((2, 64, 16, 16, 32, 1, 1, 0, 0), xoff=1)],
     None, "fallback", "alignment fallbacks: x one float off, dysn % 4 != 0 (33-channel stride on 5 x 5), a misaligned 1x1"),
]
WGRAD_IDS = [r[0] for r in WGRAD_ROWS]
EXTRA_WGRAD_ROWS = {}   # id -> descriptors of rows that other modules run through wgrad_case / WgradRun (not parametrised here)


def wgrad_descs(rid):
    return EXTRA_WGRAD_ROWS[rid] if rid in EXTRA_WGRAD_ROWS else WGRAD_ROWS[WGRAD_IDS.index(rid)][1]
# what build() is expected to choose -- WGRAD_EXPECT_BEGIN
WGRAD_EXPECT = {   # row: [(category, S in deterministic mode, S otherwise)] per descriptor
    "cat0": [(0, 1, 1), (0, 1, 1), (0, 1, 1)],
    "cat1": [(1, 1, 1), (1, 1, 1), (1, 1, 1)],
    "cat2": [(2, 2, 2), (2, 1, 1), (2, 1, 1)],
    "cat3-n5": [(3, 5, 5), (3, 5, 5), (3, 5, 5), (3, 5, 5), (3, 5, 5)],
    "cat3-n9": [(3, 9, 9), (3, 9, 9), (3, 9, 9), (3, 1, 1), (3, 2, 2)],
    "cat4": [(4, 5, 5), (4, 2, 2), (4, 1, 1)],
    "cat5": [(5, 2, 2), (5, 3, 3), (5, 2, 2)],
    "cat6": [(6, 6, 6), (6, 4, 4), (6, 1, 1)],
    "cat7": [(7, 6, 6), (7, 3, 3), (7, 1, 1)],
    "cat8": [(8, 2, 2), (8, 3, 3), (8, 1, 1)],
    "cat9": [(9, 4, 4), (9, 3, 3), (9, 2, 2)],
    "mixed": [(0, 1, 1), (9, 3, 3), (3, 5, 5), (6, 3, 3), (4, 2, 2), (2, 1, 1), (-1, 1, 1)],
    "tiny-shared": [(-1, 1, 1), (-1, 1, 1), (-1, 1, 1), (-1, 1, 1), (-1, 1, 1)],
    "shared-cat3": [(3, 5, 5), (3, 5, 5), (3, 3, 3)],
}
# WGRAD_EXPECT_END


@functools.lru_cache(maxsize=None)
def wgrad_case(rid):
    """Host buffers, float64 references and masses per gradient, the float32 oracle's deviations; shared, never modified"""
    descs = wgrad_descs(rid)
    rs = np.random.RandomState([zlib.crc32(rid.encode())])
    B, ops_, owners = {}, [], []
    for i, q in enumerate(descs):
        N, Cc, H, W, O, k, s, p, ups = q["shape"]
        OH, OW = cdiv_out(H << ups, k, s, p), cdiv_out(W << ups, k, s, p)
        xb = q["x"] or (f"x{i}", Cc, 0)
        yb = q["dy"] or (f"dy{i}", O, 0)
        if xb[0] not in B:
            B[xb[0]] = rs.normal(size=(N, xb[1], H, W)).astype(np.float32)
        if yb[0] not in B:
            B[yb[0]] = rs.normal(size=(N, yb[1], OH, OW)).astype(np.float32)
        ops_.append((xb, yb, OH, OW))
        owners.append(i if q["share"] is None else q["share"])
    grads = {}
    for o in sorted(set(owners)):
        N, Cc, H, W, O, k, s, p, ups = descs[o]["shape"]
        acc = {key: 0.0 for key in ("gW", "gb", "mW", "mb", "gW32", "gb32")}
        for i, q in enumerate(descs):
            if owners[i] != o:
                continue
            xb, yb, OH, OW = ops_[i]
            x = B[xb[0]][:, xb[2]:xb[2] + Cc]
            dy = B[yb[0]][:, yb[2]:yb[2] + O]
            for dtype, tag in ((np.float64, ""), (np.float32, "32")):
                xin = x.astype(dtype)
                xin = ops.upsample_nearest2(xin) if ups else xin
                _, gW, gb = ops.conv2d_backward(xin, np.zeros((O, Cc, k, k), dtype), dy.astype(dtype), s, p, need_gx=False)
                sc = np.dtype(dtype).type(q["scale"])
                acc["gW" + tag] = acc["gW" + tag] + sc * gW
                acc["gb" + tag] = acc["gb" + tag] + sc * gb
            xa = np.abs(x.astype(np.float64))
            xa = ops.upsample_nearest2(xa) if ups else xa
            _, mW, mb = ops.conv2d_backward(xa, np.zeros((O, Cc, k, k)), np.abs(dy.astype(np.float64)), s, p, need_gx=False)
            acc["mW"] = acc["mW"] + abs(q["scale"]) * mW
            acc["mb"] = acc["mb"] + abs(q["scale"]) * mb
        # prefill of the cleared_target = 0 runs, as test_conv2d_backward draws it
        acc["gW0"] = (rs.normal(size=acc["gW"].shape) * (np.abs(acc["gW"]).max() or 1.0)).astype(np.float32)
        acc["gb0"] = (rs.normal(size=O) * (np.abs(acc["gb"]).max() or 1.0)).astype(np.float32)
        # the float32 oracle's deviation on a cleared gradient, and adding onto the prefill in float32 (the prefill is then one of the
        # terms the entry sums: its magnitude joins the mass, as |y0| does for an accumulating output)
        for n_ in ("W", "b"):
            g64, g32, g0, m = acc["g" + n_], acc["g" + n_ + "32"], acc["g" + n_ + "0"], acc["m" + n_]
            acc["dev" + n_] = max(rel_mass(g32.astype(np.float64) - g64, m),
                                  rel_mass(((g0 + g32) - g0).astype(np.float64) - g64, m + np.abs(g0)))
        acc["has_gb"] = descs[o]["gb"]
        grads[o] = acc
    return dict(B=B, ops=ops_, owners=owners, grads=grads)


@functools.lru_cache(maxsize=None)
def wgrad_tolerances():
    worst = {"gW": 0.0, "gb": 0.0}
    for rid in WGRAD_IDS:
        for g in wgrad_case(rid)["grads"].values():
            worst["gW"] = max(worst["gW"], g["devW"])
            if g["has_gb"]:
                worst["gb"] = max(worst["gb"], g["devb"])
    return {"gW": tolerance(worst["gW"]), "gb": tolerance(worst["gb"]), "worst32": worst}


class WgradRun:
    """The device side of a row: operands uploaded once; call(cleared) re-fills the gradients and runs the op (on ctx instead of the
    default context, where one is given)"""

    def __init__(self, dbm, rid, ctx=None):
        self.d, self._lib, self.ctx = dbm if ctx is None else (dbm[0], dbm[1], ctx)
        self.descs = wgrad_descs(rid)
        self.case = wgrad_case(rid)
        d, case = self.d, self.case
        self.dev, self.ptr = {}, {}
        off = {}
        for q, (xb, yb, _, _) in zip(self.descs, case["ops"]):
            if q["xoff"]:
                off[xb[0]] = q["xoff"]
        for name, host in case["B"].items():
            o = off.get(name, 0)
            self.dev[name] = d.to_device(np.concatenate([np.zeros(o, np.float32), host.reshape(-1)]))
            self.ptr[name] = self.dev[name].ptr + 4 * o
        self.gW = {o: d.to_device(g["gW0"]) for o, g in case["grads"].items()}
        self.gb = {o: d.to_device(g["gb0"]) for o, g in case["grads"].items() if g["has_gb"]}
        n = len(self.descs)
        self.arr = (self._lib.WgradDesc * n)()
        for i, (q, (xb, yb, OH, OW)) in enumerate(zip(self.descs, case["ops"])):
            N, Cc, H, W, O, k, s, p, ups = q["shape"]
            a, o = self.arr[i], case["owners"][i]
            a.x, a.xsn = self.ptr[xb[0]] + 4 * xb[2] * H * W, xb[1] * H * W
            a.dy, a.dysn = self.ptr[yb[0]] + 4 * yb[2] * OH * OW, yb[1] * OH * OW
            a.N, a.C, a.H, a.W, a.O, a.k, a.stride, a.pad, a.ups = N, Cc, H, W, O, k, s, p, ups
            a.scale = q["scale"]
            a.gW = self.gW[o].ptr
            a.gb = self.gb[o].ptr if o in self.gb else None

    def call(self, cleared):
        """-> ({owner: (gW - prefill, gb - prefill or None)} as float64, raw bits, categories, S)"""
        n = len(self.descs)
        for o, g in self.case["grads"].items():
            self.gW[o].set(np.zeros_like(g["gW0"]) if cleared else g["gW0"])
            if o in self.gb:
                self.gb[o].set(np.zeros_like(g["gb0"]) if cleared else g["gb0"])
        cat, S = (C.c_int * n)(), (C.c_int * n)()
        self._lib.check(self._lib.lib().dbm_op_conv2d_wgrad_batch(self.ctx.handle, self.arr, n, int(cleared), cat, S), self.ctx.handle)
        out, raw = {}, []
        for o, g in self.case["grads"].items():
            w = self.gW[o].get()
            b = self.gb[o].get() if o in self.gb else None
            raw += [bits(w)] + ([bits(b)] if b is not None else [])
            out[o] = (w.astype(np.float64) - (0.0 if cleared else g["gW0"]), None if b is None else b.astype(np.float64) - (0.0 if cleared else g["gb0"]))
        return out, raw, list(cat), list(S)

    def errors(self, out, cleared):
        eW = eb = 0.0
        for o, g in self.case["grads"].items():
            w, b = out[o]
            eW = max(eW, rel_mass(w - g["gW"], g["mW"] + (0.0 if cleared else np.abs(g["gW0"]))))
            if b is not None:
                eb = max(eb, rel_mass(b - g["gb"], g["mb"] + (0.0 if cleared else np.abs(g["gb0"]))))
        return eW, eb


def restore_deterministic(ctx):
    from deepbedmap_amd import srgan

    srgan._applied_deterministic[0] = None   # what srgan.apply_config sets, so that later modules see the default
    srgan.apply_config(ctx)


@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("cleared", [0, 1])
@pytest.mark.parametrize("rid", WGRAD_IDS)
def test_wgrad_batch(dbm, rid, cleared, det):
    d, _lib, ctx = dbm
    _, descs, _, special, why = WGRAD_ROWS[WGRAD_IDS.index(rid)]
    tol = wgrad_tolerances()
    try:
        _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
        run = WgradRun(dbm, rid)
        out, raw, cat, S = run.call(cleared)
        eW, eb = run.errors(out, cleared)
        print(f"{rid} cleared={cleared} det={det}: cat {cat} S {S}  gW {eW:.3e} (tol {tol['gW']:.3e})  gb {eb:.3e} (tol {tol['gb']:.3e})")
        if special == "fallback":
            assert all(c not in (3, 9) for c in cat), cat
        else:
            want = WGRAD_EXPECT[rid]
            assert cat == [e[0] for e in want], (why, cat)
            assert S == [e[1] if det else e[2] for e in want], (why, S)
        assert eW <= tol["gW"], (eW, tol["gW"])
        assert eb <= tol["gb"], (eb, tol["gb"])
        if det:
            _, raw2, cat2, S2 = run.call(cleared)
            assert (cat2, S2) == (cat, S)
            assert all(np.array_equal(a, b) for a, b in zip(raw, raw2)), "deterministic mode: a repeated call gave other bits"
    finally:
        restore_deterministic(ctx)


@pytest.mark.parametrize("rid", ["cat3-n9", "mixed"])
def test_wgrad_batch_replans_when_the_mode_switches(dbm, rid):
    """The op keeps the batch of the previous call with the same descriptors, as the training step keeps its batches: switching the
    mode (and cleared_target) in between goes through the re-plan in WgradBatch::launch; every call must be right, and the
    deterministic calls before and after must agree bit for bit"""
    d, _lib, ctx = dbm
    tol = wgrad_tolerances()
    try:
        run = WgradRun(dbm, rid)
        seen = {}
        for det, cleared in [(1, 0), (0, 0), (1, 0), (1, 1), (0, 1), (1, 1)]:
            _lib.check(_lib.lib().dbm_set_deterministic(ctx.handle, det), ctx.handle)
            out, raw, cat, S = run.call(cleared)
            eW, eb = run.errors(out, cleared)
            assert eW <= tol["gW"] and eb <= tol["gb"], (det, cleared, eW, eb)
            if det:
                if cleared in seen:
                    assert all(np.array_equal(a, b) for a, b in zip(raw, seen[cleared])), (det, cleared)
                seen[cleared] = raw
    finally:
        restore_deterministic(ctx)
