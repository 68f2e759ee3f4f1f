"""Regenerates tests/golden/esrgan_full.partNN.npz: oracle outputs at BASELINE.json's FULL configuration sizes.

    python tests/golden/make_golden_full.py            # ~5 minutes on 8 cores, ~12 GB peak

The reference's numerics live in Chainer, which cannot be imported in this image, so -- like
esrgan_small.npz -- these vectors come from the repo's own oracle (pinned by the reference's known answers,
tests/test_oracle_kats.py).  What they add: the HIP path is compared with the oracle at the sizes the benchmark runs
(192 resident workgroups of the persistent trunk kernels, three bands per image, prefetched forward, merged
discriminator weight-gradient launches), where running the oracle inside the GPU test would take minutes.

  c3  BASELINE config 3: full ESRGAN iteration, batch 64, 12 RRDB (srgan_train.py:1084-1263): generator forward,
      D-step [loss, accuracy], G-step [loss, psnr, ssim], every gradient of both models, BatchNorm running statistics;
  c3lin  the G-step of the same configuration with the reference's own initialisation (HeNormal 0.1): every
      pre-activation is dominated by its bias, no LeakyReLU slope hangs on a rounding error, and the float32 oracle is
      a 5e-4 reference for every gradient through the persistent backward kernel at full occupancy;
  c2  BASELINE config 2: generator only, 16 RRDB, batch 32, pixel-L1 loss (F.mean_absolute_error): forward, loss,
      every gradient;
  c5  BASELINE config 5: ONE interior 288 x 288 crop of the continent sweep (deepbedmap.py:706-728) -> 1144 x 1144,
      fp32 forward (the reference for the bf16 sweep mode as well).

Large tensors are stored as a digest: a seeded sample of entries, the l2 norm, the largest magnitude and four random
+-1 projections in float64 (a projection error relative to the l2 norm IS the relative rms error of the tensor, and
any misplaced / missing block of contributions shows up in it).  Weights and inputs are NOT stored: they are seeded
(`models_c3` ..., `arrays`) and rebuilt by the test through the same functions.

Conditioning.  At batch 64 a training iteration is NOT reproducible to 1e-4 by ANY two float32 implementations: with
~10^7 activations per layer a handful sit within one rounding error of zero, their LeakyReLU slope flips between 1 and
0.2 from one summation order to the next, and BatchNorm's backward pass (which removes the batch-constant part of the
gradient) amplifies what is left.  The float32 oracle itself moves by up to 1e-2 (max-norm of a weight gradient) when
its arithmetic is switched to float64.  c3 therefore stores the FLOAT64 oracle as the reference and, per tensor, how
far the float32 oracle is from it (`.../dev`): the GPU test requires the HIP path to be as close to the float64
numbers as the float32 CPU restatement is (a small multiple of `dev`, never below the plain tolerance).  The
generator's weights are HeNormal x 8 there, so that the fakes carry texture (std 0.47 around a mean of 0.19); with
the reference's own 0.1 scale the fakes are constant to 1e-3, BatchNorm on the fake batch divides by that, and even
the two oracles disagree by 50 % on the discriminator's gradients.  The generator's gradients of that configuration
carry a second, coherent kind of noise: ONE flipped slope or bilinear cell near the output changes the whole trunk
gradient of its image by tens of per cent, i.e. every trunk tensor by a few 1e-3 of the batch sum -- the test allows
a multiple of the WORST deviation the float32 oracle shows on any tensor there, and the tight check of the backward
kernels is c3lin.

    python tests/golden/make_golden_full.py c3lin c2      # recompute only these, keep the rest of the file

Round 3 -- tests/golden/esrgan_dem.partNN.npz (`python tests/golden/make_golden_full.py dem dem5 dlin`):

  dem   the full iteration of config 3 at the REFERENCE'S DATA RANGE (SURVEY 8d "DEM-like"): the reference feeds raw metres,
        m/yr and kg/m2/yr (deepbedmap.py:164-169 gap-fills BEDMAP2 with -5000 m; paper/tc-2020-74.tex:192-197): X ~ U[-2000, 2000]
        with -5000 blocks, W1 ~ U[0, 4000], W2 ~ U[0, 1000], W3 ~ U[0, 500].  The weights are scaled so that activations
        STAY in that range through the network the way a trained model's do (`models_dem`), and the target Y is correlated
        with the prediction (0.8 x the oracle's float64 forward + U[-300, 300] m, stored), so that the SSIM term works on
        tiles whose mean (thousands of metres) dwarfs their variance -- the regime where E[x^2] - mu^2 in float32 fails;
  dem5  one interior 288 x 288 crop of the continent sweep at the same data range (fp32 oracle; the bf16 mode's error is
        reported in metres against it);
  dlin  the D-step of config 3 with a discriminator whose every LeakyReLU input is dominated by its bias / beta
        (no slope hangs on a rounding error, cf. c3lin): the float32 oracle is a tight reference for EVERY discriminator
        gradient, BatchNorm running statistic and the loss at batch 64; mid-size tensors are stored in full.

Round 4 -- `python tests/golden/make_golden_full.py demlin` (also esrgan_dem):

  demlin  the G-step of config 3 at the DATA RANGE with a generator in the linear regime (c3lin carried to metres: the
          reference's HeNormal 0.1 weights, biases ~ N(0, 0.1 x 2000 m) so that every pre-activation is dominated by its bias
          at this magnitude too, offset convolutions scaled back to offsets of a fraction of a pixel): the float32 oracle is a
          5e-4 reference for EVERY generator gradient on inputs in metres (`dem` holds them to a multiple of the float32
          oracle's own deviation only).
"""
import glob
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import model as omodel  # noqa: E402
from oracle import train as otrain  # noqa: E402

# a fixture set is stored as <PATH>.partNN.npz, each part below 1 MiB: `load(PATH)` / `save(PATH, arrays)`
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "esrgan_full")
PART_BYTES = 900_000   # uncompressed array bytes per part (float data barely compresses: the file stays below 1 MiB)
NSAMPLE = 512   # entries kept per tensor (whole tensor if smaller)
NPROJ = 4
ALPHA, EPS = 1e-4, 1e-8


def parts(path):
    return sorted(glob.glob(glob.escape(path) + ".part[0-9][0-9].npz"))


def load(path):
    """Every array of the fixture set `path` (all of its parts), by key."""
    out = {}
    for p in parts(path):
        with np.load(p) as f:
            out.update({k: f[k] for k in f.files})
    assert out, f"no {path}.partNN.npz"
    return out


def save(path, arrays):
    """Writes `arrays` as the fixture set `path`, keys in order, a new part whenever PART_BYTES would be exceeded."""
    for p in parts(path):
        os.remove(p)
    groups, n = [{}], 0
    for k, v in arrays.items():
        if groups[-1] and n + v.nbytes > PART_BYTES:
            groups.append({})
            n = 0
        groups[-1][k] = v
        n += v.nbytes
    for i, g in enumerate(groups):
        np.savez_compressed(f"{path}.part{i:02d}.npz", **g)
        assert os.path.getsize(f"{path}.part{i:02d}.npz") < 1 << 20, (path, i, list(g))


# ---- seeded inputs and weights (shared with tests/test_gpu_fullsize.py) ----
def arrays(n, seed, h=11, w=11):
    """One independent stream per array (the reference's own fixture seeds all five alike, srgan_train.py:1101-1105,
    which makes X == W3: useless for catching a swapped branch)."""
    r = [np.random.RandomState(seed + i) for i in range(5)]
    f = np.float32
    return {"X": r[0].rand(n, 1, h, w).astype(f), "W1": r[1].rand(n, 1, 10 * h, 10 * w).astype(f),
            "W2": r[2].rand(n, 2, 2 * h, 2 * w).astype(f), "W3": r[3].rand(n, 1, h, w).astype(f),
            "Y": r[4].rand(n, 1, 4 * (h - 2), 4 * (w - 2)).astype(f)}


def oracle_generator(n_blocks, seed, bias_noise=0.1, scale=1.0):
    """The reference's initialisation (HeNormal(0.1), srgan_train.py:220), optionally scaled, plus non-zero biases."""
    g = omodel.GeneratorModel(num_residual_blocks=n_blocks, seed=seed)
    r = np.random.RandomState(seed + 1)
    for k in sorted(g.params):
        if k.endswith("/W"):
            g.params[k] *= np.float32(scale)
        else:
            g.params[k] += r.normal(0, bias_noise, g.params[k].shape).astype(np.float32)
    return g


def to_float64(model):
    """The same model (bitwise the same float32 parameter values) computing in float64."""
    model.dtype = np.float64
    for k in model.params:
        model.params[k] = model.params[k].astype(np.float64)
    for k in getattr(model, "persistent", {}):
        model.persistent[k] = np.asarray(model.persistent[k], np.float64 if not k.endswith("/N") else np.int64)
    return model


def oracle_discriminator(seed):
    d = omodel.DiscriminatorModel(seed=seed)
    r = np.random.RandomState(seed + 1)
    for k in sorted(d.params):
        if k.endswith("/W"):
            d.params[k] *= np.float32(3.0)  # logits of an untrained D are ~1e-3 otherwise
        elif k.endswith("gamma"):
            d.params[k] += r.normal(0, 0.2, d.params[k].shape).astype(np.float32)
        else:
            d.params[k] += r.normal(0, 0.1, d.params[k].shape).astype(np.float32)
    return d


def models_c3():
    return oracle_generator(12, 101, scale=8.0), oracle_discriminator(202)


def models_c3lin():
    return oracle_generator(12, 505), oracle_discriminator(606)


def models_c2():
    return oracle_generator(16, 303)


def models_c5():
    return oracle_generator(12, 404)


def target_c2():
    return np.random.RandomState(77).rand(32, 1, 36, 36).astype(np.float32)


# ---- the reference's data range (SURVEY 8d "DEM-like"; deepbedmap.py:164-169, 663-665) ----
PATH_DEM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "esrgan_dem")


def arrays_dem(n, seed, h=11, w=11):
    """Raw physical units as the reference feeds them: X = BEDMAP2 bed elevation [m] with -5000 m gap-fill blocks
    (deepbedmap.py:164-169), W1 = ice surface elevation [m], W2 = ice velocity [m/yr], W3 = accumulation [kg/m2/yr]
    (W1..W3 clipped to >= 0 by the caller, deepbedmap.py:663-665).  Y here is a placeholder of the same range: the
    fixtures replace it by a target correlated with the prediction (`dem/Y`)."""
    r = [np.random.RandomState(seed + i) for i in range(6)]
    f = np.float32
    a = {"X": r[0].uniform(-2000, 2000, (n, 1, h, w)).astype(f), "W1": r[1].uniform(0, 4000, (n, 1, 10 * h, 10 * w)).astype(f),
         "W2": r[2].uniform(0, 1000, (n, 2, 2 * h, 2 * w)).astype(f), "W3": r[3].uniform(0, 500, (n, 1, h, w)).astype(f),
         "Y": r[4].uniform(-2000, 2000, (n, 1, 4 * (h - 2), 4 * (w - 2))).astype(f)}
    for i in range(0, n, 3):  # gap-fill blocks in every third tile (a few per large crop)
        for _ in range(1 if h < 64 else 6):
            bh, bw = r[5].randint(2, max(3, h // 4)), r[5].randint(2, max(3, w // 4))
            y0, x0 = r[5].randint(0, h - bh + 1), r[5].randint(0, w - bw + 1)
            a["X"][i, 0, y0:y0 + bh, x0:x0 + bw] = -5000.0
    return a


def oracle_generator_dem(n_blocks, seed):
    """A generator whose activations stay at the data's magnitude (O(10^3)) from the input block to the output, like a
    trained model's: the layers on the main path (input block, pre-residual, upsampling, deformable GEMMs) are
    variance-preserving (HeNormal x 10 = He scale 1), the residual branches (trunk, post-residual) contribute a third of their
    input per conv (x 3), and the offset convolutions produce offsets of about a pixel (x 10 x 1e-3) instead of thousands."""
    g = omodel.GeneratorModel(num_residual_blocks=n_blocks, seed=seed)
    r = np.random.RandomState(seed + 1)
    for k in sorted(g.params):
        if k.endswith("/W"):
            sc = 3.0 if (k.startswith("residual_network/") or k.startswith("post_residual")) else 10.0
            if "offset_conv" in k:
                sc *= 1e-3
            g.params[k] *= np.float32(sc)
        else:
            g.params[k] += r.normal(0, 0.1, g.params[k].shape).astype(np.float32)
    return g


def models_dem():
    """The discriminator is the LINEAR-regime one (oracle_discriminator_lin, scaled for images in metres): at this data range
    the generator's own float32 rounding (2e-5 of a +-9000 m output, ten times c3's) flips ~100 LeakyReLU slopes of a
    natural discriminator from one implementation to the next and its gradients then agree to 20 % only (measured:
    identical fakes -> 1e-5, fakes perturbed by 2e-5 of the range -> 0.03 median / 0.19 worst); in the linear regime the
    same perturbation moves them by < 1e-4, so every discriminator gradient is held to 5e-4 here too."""
    return oracle_generator_dem(12, 707), oracle_discriminator_lin(808, img_sigma=2000.0)


def models_dem5():
    return oracle_generator_dem(12, 909)


DEMLIN_S = 2000.0  # magnitude of the data (metres)


def oracle_generator_demlin(n_blocks, seed):
    """c3lin's generator carried to the data range: the network is positively homogeneous in (inputs, biases) -- convolutions and
    LeakyReLU are -- so the reference initialisation with biases ~ N(0, 0.1 x S) sees inputs of magnitude S exactly as c3lin's
    sees U[0, 1): pre-activations dominated by their bias, no slope on a rounding edge.  The deformable layers are the exception
    (their offsets are pixels, not metres): the offset convolutions are scaled by 1 / S so that the offsets stay what they are
    in c3lin, a fraction of a pixel."""
    g = oracle_generator(n_blocks, seed, bias_noise=0.1 * DEMLIN_S)
    for k in sorted(g.params):
        if "offset_conv" in k:
            g.params[k] = (g.params[k] / np.float32(DEMLIN_S)).astype(np.float32)
    return g


def models_demlin():
    return oracle_generator_demlin(12, 1505), oracle_discriminator_lin(1606, img_sigma=2000.0)


def oracle_discriminator_lin(seed, img_sigma=0.29):
    """A discriminator in the LINEAR regime (img_sigma: standard deviation of the images it will see -- 0.29 for U[0, 1),
    ~2000 for elevations in metres: conv_layer0's bias is scaled with it, everything behind BatchNorm is scale free): every LeakyReLU input is held away from zero by its bias / beta
    (pre-activation = gamma x_hat + beta with gamma ~ 1, |beta| ~ 4: the density of values within a rounding error of
    zero is 1.3e-4 of the natural one -- ~1e-4 expected slope flips per batch-64 iteration instead of ~10), so float32
    implementations agree to ~1e-6 on every gradient and the float32 oracle is a TIGHT reference at full size.
    A constant per-channel offset would, through the zero padding, turn into positional variance that BatchNorm then
    normalises by (the per-sample signal dies within a few layers): every convolution / linear weight is therefore made
    orthogonal, tap by tap, to the vector of its input channels' means (= lrelu(beta) of the layer below), so that only
    the variation of the activations travels."""
    d = omodel.DiscriminatorModel(seed=seed)
    r = np.random.RandomState(seed + 1)
    P = d.params
    lrelu = lambda v: np.where(v > 0, v, 0.2 * v)  # noqa: E731
    signed = lambda shape, lo, hi: (r.randint(0, 2, shape) * 2 - 1) * r.uniform(lo, hi, shape)  # noqa: E731
    W0 = P["conv_layer0/W"].astype(np.float64) * 3.0
    W0 -= W0.mean(axis=(1, 2, 3), keepdims=True)  # zero-sum kernels: the image's mean level does not reach conv_layer1
    b0 = signed((64,), 1.5, 2.0) * (img_sigma / 0.29)  # (|W0 * img| has sigma ~0.12 at img_sigma 0.29: the bias is > 12 sigma)
    P["conv_layer0/W"], P["conv_layer0/b"] = W0.astype(np.float32), b0.astype(np.float32)
    m = lrelu(b0)
    for i in range(1, 10):
        W = P[f"conv_layer{i}/W"].astype(np.float64) * 3.0
        coef = np.einsum("ocyx,c->oyx", W, m) / float((m * m).sum())
        W -= coef[:, None, :, :] * m[None, :, None, None]
        P[f"conv_layer{i}/W"] = W.astype(np.float32)
        c = W.shape[0]
        beta = signed((c,), 3.5, 4.5)
        P[f"batch_norm{i}/gamma"] = r.uniform(0.8, 1.2, (c,)).astype(np.float32)
        P[f"batch_norm{i}/beta"] = beta.astype(np.float32)
        m = lrelu(beta)
    W1 = P["linear_1/W"].astype(np.float64) * 10.0
    W1 -= np.outer(W1 @ m / float(m @ m), m)
    P["linear_1/W"] = W1.astype(np.float32)
    P["linear_1/b"] = signed((100,), 3.5, 4.5).astype(np.float32)
    P["linear_2/W"] = (P["linear_2/W"].astype(np.float64) * 10.0).astype(np.float32)  # logits differ by O(1) between samples
    P["linear_2/b"] = r.normal(0, 0.1, (1,)).astype(np.float32)
    return d


def models_dlin():
    return oracle_generator(12, 101, scale=8.0), oracle_discriminator_lin(1202)


DLIN_FLOOR = 1e-3  # gradients below this fraction of the largest one carry rounding noise only (three are exactly zero in theory)
DLIN_FULL = ("conv_layer0/W", "conv_layer0/b", "conv_layer1/W", "conv_layer2/W", "linear_1/W", "linear_1/b", "linear_2/W",
             "linear_2/b") + tuple(f"batch_norm{i}/{p}" for i in range(1, 10) for p in ("gamma", "beta"))


# ---- digests ----
def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def digest(name, a):
    """(sample values float32[min(size, NSAMPLE)], stats float64[2 + NPROJ] = l2, max|.|, projections)."""
    a = np.asarray(a)
    flat = a.reshape(-1)
    r = _rng(name)
    idx = np.arange(flat.size) if flat.size <= NSAMPLE else np.sort(r.choice(flat.size, NSAMPLE, replace=False))
    f64 = flat.astype(np.float64)
    stats = [float(np.sqrt((f64 * f64).sum())), float(np.abs(f64).max())]
    for _ in range(NPROJ):
        sign = r.randint(0, 2, flat.size).astype(np.float64) * 2.0 - 1.0
        stats.append(float((f64 * sign).sum()))
    return flat[idx].astype(np.float32), np.array(stats, np.float64)


def digest_dict(prefix, tensors):
    """name-sorted digests of a dict of arrays, packed into two arrays (+ the offsets of each tensor's sample)."""
    samples, stats, offs = [], [], [0]
    for k in sorted(tensors):
        s, st = digest(prefix + k, tensors[k])
        samples.append(s)
        stats.append(st)
        offs.append(offs[-1] + s.size)
    return {prefix + "samples": np.concatenate(samples), prefix + "stats": np.stack(stats),
            prefix + "offsets": np.array(offs, np.int64)}


# linear_2/b of the discriminator: the two batches' loss gradients cancel EXACTLY in theory (symmetric relativistic loss); what a
# float32 run leaves is the rounding of 128 terms of +-1/128, a few 1e-8, which changes with the last bit of any logit, i.e. with
# the summation order of any convolution.  It is held to this fraction of the largest gradient instead of the common floor.
ZERO_GRAD_FLOORS = {"linear_2/b": 4e-3}


def digest_errors(gold, prefix, tensors, floor=1e-6, floors=None):
    """name -> (sample error, projection error) of a dict of arrays against a stored digest_dict: the sample error is
    max-norm relative to the tensor's largest magnitude, the projection error (incl. the l2 norm itself) relative to
    its l2 norm = the relative rms error.  Neither scale is finer than `floor` x the largest magnitude of the whole
    dict (gradients that are exactly zero in theory only carry rounding noise)."""
    names = sorted(tensors)
    stats, offs, samples = gold[prefix + "stats"], gold[prefix + "offsets"], gold[prefix + "samples"]
    assert len(names) == len(stats), (len(names), len(stats))
    gmax = float(stats[:, 1].max())
    out = {}
    for i, k in enumerate(names):
        s, st = digest(prefix + k, tensors[k])
        ref_s = samples[offs[i]:offs[i + 1]]
        assert s.shape == ref_s.shape, k
        fl = max(floor, floors.get(k, 0.0)) if floors else floor
        scale = max(float(stats[i, 1]), fl * gmax)
        e_s = float(np.abs(s.astype(np.float64) - ref_s).max()) / scale
        l2 = max(float(stats[i, 0]), fl * gmax * np.sqrt(np.asarray(tensors[k]).size))
        e_p = max(float(np.abs(st[2:] - stats[i, 2:]).max()), abs(st[0] - stats[i, 0])) / l2
        out[k] = (e_s, e_p)
    return out


def check_digest_dict(gold, prefix, tensors, tol_sample, tol_proj, floor=1e-6, dev_factor=0.0, floors=None):
    """Compares a dict of arrays with a stored digest_dict.  Returns the worst (error / tolerance, name, what).
    dev_factor > 0: a tensor's tolerance is max(tol, dev_factor x the float32 oracle's own deviation from this float64
    reference), stored as `prefix + "dev"` (see the module docstring, Conditioning)."""
    errs = digest_errors(gold, prefix, tensors, floor, floors)
    dev = gold[prefix + "dev"] if dev_factor > 0 else None
    worst = (0.0, "", "")
    for i, k in enumerate(sorted(tensors)):
        ts = max(tol_sample, dev_factor * dev[i, 0]) if dev is not None else tol_sample
        tp = max(tol_proj, dev_factor * dev[i, 1]) if dev is not None else tol_proj
        for e, what in ((errs[k][0] / ts, "sample"), (errs[k][1] / tp, "projection")):
            if e > worst[0]:
                worst = (e, k, what)
    return worst


def with_dev(gold_part, prefix, tensors32, floor):
    """Adds `prefix + "dev"` (n_tensors, 2): the float32 oracle's deviation from the float64 digests in gold_part."""
    errs = digest_errors(gold_part, prefix, tensors32, floor)
    gold_part[prefix + "dev"] = np.array([errs[k] for k in sorted(tensors32)], np.float64)
    return gold_part


# ---- the three configurations ----
D_FLOOR, G_FLOOR = 1e-4, 1e-6


def _iteration_c3(f64):
    a = arrays(64, 4200)
    g, d = models_c3()
    if f64:
        to_float64(g), to_float64(d)
        a = {k: v.astype(np.float64) for k, v in a.items()}
    out = {"g_forward": g.forward(a["X"], a["W1"], a["W2"], a["W3"])}
    out["d_step"] = np.array(otrain.train_eval_discriminator(a, g, d, otrain.Adam(d.params, alpha=ALPHA, eps=EPS)), np.float64)
    out["gradD"] = {k: v.copy() for k, v in d.grads.items()}
    out["persD"] = {k: np.asarray(v, np.float64) for k, v in d.persistent.items() if not k.endswith("/N")}
    out["g_step"] = np.array(otrain.train_eval_generator(a, g, d, otrain.Adam(g.params, alpha=ALPHA, eps=EPS)), np.float64)
    out["gradG"] = {k: v.copy() for k, v in g.grads.items()}
    return out


def compute_c3():
    """Reference = the float64 oracle; `dev` = how far the float32 oracle is from it (see Conditioning above)."""
    r64, r32 = _iteration_c3(True), _iteration_c3(False)
    y64 = r64["g_forward"]
    out = {"c3/g_forward": y64.astype(np.float32),
           "c3/g_forward_dev": np.array(np.abs(r32["g_forward"] - y64).max() / np.abs(y64).max()),
           "c3/d_step": r64["d_step"], "c3/d_step_f32": r32["d_step"],
           "c3/g_step": r64["g_step"], "c3/g_step_f32": r32["g_step"]}
    for name, floor in (("gradD", D_FLOOR), ("persD", G_FLOOR), ("gradG", G_FLOOR)):
        part = digest_dict(f"c3/{name}/", r64[name])
        out.update(with_dev(part, f"c3/{name}/", r32[name], floor))
    return out


def compute_c3lin():
    a = arrays(64, 6200)
    g, d = models_c3lin()
    out = {"c3lin/g_step": np.array(otrain.train_eval_generator(a, g, d, otrain.Adam(g.params, alpha=ALPHA, eps=EPS)), np.float64)}
    out.update(digest_dict("c3lin/gradG/", g.grads))
    return out


def compute_c2():
    a = arrays(32, 3100)
    g = models_c2()
    t = target_c2()
    y = g.forward(a["X"], a["W1"], a["W2"], a["W3"], keep=True)
    out = {"c2/g_forward": y, "c2/loss": np.array(float(np.abs(y - t).mean()), np.float64)}
    gy = (np.sign(y - t) / np.float32(y.size)).astype(np.float32)  # F.mean_absolute_error backward
    out.update(digest_dict("c2/gradG/", g.backward(gy)))
    return out


C5_STRIDE, C5_BLOCK = 8, 64


def compute_c5():
    a = arrays(1, 5100, h=288, w=288)
    g = models_c5()
    y = g.forward(a["X"], a["W1"], a["W2"], a["W3"])  # (1, 1, 1144, 1144)
    s, st = digest("c5/y", y)
    c = y.shape[2] // 2 - C5_BLOCK // 2
    return {"c5/grid": y[0, 0, ::C5_STRIDE, ::C5_STRIDE].copy(), "c5/centre": y[0, 0, c:c + C5_BLOCK, c:c + C5_BLOCK].copy(),
            "c5/samples": s, "c5/stats": st, "c5/shape": np.array(y.shape, np.int64)}


def _iteration_dem(f64, Y=None):
    a = arrays_dem(64, 7100)
    g, d = models_dem()
    if f64:
        to_float64(g), to_float64(d)
        a = {k: v.astype(np.float64) for k, v in a.items()}
    out = {"g_forward": g.forward(a["X"], a["W1"], a["W2"], a["W3"])}
    if Y is None:  # the target: correlated with the prediction, a few hundred metres of independent relief on top
        Y = (0.8 * out["g_forward"] + np.random.RandomState(7199).uniform(-300, 300, out["g_forward"].shape)).astype(np.float32)
    a["Y"] = Y.astype(a["X"].dtype)
    out["Y"] = Y
    out["d_step"] = np.array(otrain.train_eval_discriminator(a, g, d, otrain.Adam(d.params, alpha=ALPHA, eps=EPS)), np.float64)
    out["gradD"] = {k: v.copy() for k, v in d.grads.items()}
    out["persD"] = {k: np.asarray(v, np.float64) for k, v in d.persistent.items() if not k.endswith("/N")}
    out["g_step"] = np.array(otrain.train_eval_generator(a, g, d, otrain.Adam(g.params, alpha=ALPHA, eps=EPS)), np.float64)
    out["gradG"] = {k: v.copy() for k, v in g.grads.items()}
    return out


def compute_dem():
    r64 = _iteration_dem(True)
    r32 = _iteration_dem(False, Y=r64["Y"])
    y64 = r64["g_forward"]
    out = {"dem/g_forward": y64.astype(np.float32), "dem/Y": r64["Y"],
           "dem/g_forward_dev": np.array(np.abs(r32["g_forward"] - y64).max() / np.abs(y64).max()),
           "dem/d_step": r64["d_step"], "dem/d_step_f32": r32["d_step"],
           "dem/g_step": r64["g_step"], "dem/g_step_f32": r32["g_step"]}
    for name, floor in (("gradD", DLIN_FLOOR), ("persD", G_FLOOR), ("gradG", G_FLOOR)):
        part = digest_dict(f"dem/{name}/", r64[name])
        out.update(with_dev(part, f"dem/{name}/", r32[name], floor))
    print("dem: forward dev", float(out["dem/g_forward_dev"]), "range", float(y64.min()), float(y64.max()), "d", r64["d_step"],
          r32["d_step"], "g", r64["g_step"], r32["g_step"], "gradD dev", out["dem/gradD/dev"].max(0), "gradG dev",
          out["dem/gradG/dev"].max(0), "persD dev", out["dem/persD/dev"].max(0), flush=True)
    return out


def compute_dem5():
    a = arrays_dem(1, 7500, h=288, w=288)
    g = models_dem5()
    y = g.forward(a["X"], a["W1"], a["W2"], a["W3"])  # (1, 1, 1144, 1144), metres
    s, st = digest("dem5/y", y)
    c = y.shape[2] // 2 - C5_BLOCK // 2
    print("dem5: range", float(y.min()), float(y.max()), "std", float(y.std()), flush=True)
    return {"dem5/grid": y[0, 0, ::C5_STRIDE, ::C5_STRIDE].copy(), "dem5/centre": y[0, 0, c:c + C5_BLOCK, c:c + C5_BLOCK].copy(),
            "dem5/samples": s, "dem5/stats": st, "dem5/shape": np.array(y.shape, np.int64),
            "dem5/std": np.array(float(y.std()), np.float64)}


def _dstep_dlin(f64):
    a = arrays(64, 8200)
    g, d = models_dlin()
    if f64:
        to_float64(g), to_float64(d)
        a = {k: v.astype(np.float64) for k, v in a.items()}
    m = np.array(otrain.train_eval_discriminator(a, g, d, otrain.Adam(d.params, alpha=ALPHA, eps=EPS)), np.float64)
    return m, {k: v.copy() for k, v in d.grads.items()}, {k: np.asarray(v, np.float64) for k, v in d.persistent.items()
                                                            if not k.endswith("/N")}


def compute_dlin():
    """Reference = the float32 oracle (what the HIP path restates); its distance from the float64 oracle is recorded and
    must be tiny -- that is what makes this fixture a TIGHT check."""
    m64, g64, p64 = _dstep_dlin(True)
    m32, g32, p32 = _dstep_dlin(False)
    out = {"dlin/d_step": m32, "dlin/d_step_f64": m64}
    out.update(digest_dict("dlin/gradD/", g32))
    out.update(digest_dict("dlin/persD/", p32))
    part64 = digest_dict("dlin/gradD/", g64)
    dev = with_dev(part64, "dlin/gradD/", g32, DLIN_FLOOR)["dlin/gradD/dev"]
    out["dlin/gradD/dev"] = dev
    for k in DLIN_FULL:
        out["dlin/full/" + k] = g32[k].astype(np.float32)
    print("dlin: d_step", m32, m64, "worst float32-vs-float64 deviation (sample, projection)", dev.max(0), flush=True)
    print("dlin: per tensor", {k: tuple(float(f"{v:.1e}") for v in dev[i]) for i, k in enumerate(sorted(g32))}, flush=True)
    assert dev.max() < 2e-4, "dlin is meant to be well conditioned"  # (measured: <= 2e-5 on every conv / linear weight, 1.3e-4 on conv_layer0/b)
    return out


def _gstep_demlin(f64, Y=None):
    a = arrays_dem(64, 9100)
    g, d = models_demlin()
    if f64:
        to_float64(g), to_float64(d)
        a = {k: v.astype(np.float64) for k, v in a.items()}
    y = g.forward(a["X"], a["W1"], a["W2"], a["W3"])
    if Y is None:  # the target: correlated with the prediction + independent relief of a third of its spread
        spread = float(np.asarray(y, np.float64).std())
        Y = (0.8 * y + np.random.RandomState(9199).uniform(-0.5 * spread, 0.5 * spread, y.shape)).astype(np.float32)
    a["Y"] = Y.astype(a["X"].dtype)
    m = np.array(otrain.train_eval_generator(a, g, d, otrain.Adam(g.params, alpha=ALPHA, eps=EPS)), np.float64)
    return m, {k: v.copy() for k, v in g.grads.items()}, Y, np.asarray(y)


def compute_demlin():
    """Reference = the FLOAT64 oracle.  No LeakyReLU slope hangs on a rounding error here (the trunk's gradients of the float32
    oracle agree with it to 1.5e-4), but the float32 ORACLE is not a tight reference for the layers behind the loss: the
    prediction is 160 m +- 3 m per tile, and the SSIM term's sigma^2 = E[x^2] - mu^2 -- the formula of ssim-chainer, restated as
    is -- loses its digits in float32 (the two oracles' SSIM values differ by 3 %, their tail-layer gradients by up to 7e-3: `dev`).
    The HIP path computes the windows on mean-shifted tiles (norm_loss.hip) and is held to 5e-4 of the float64 numbers on EVERY
    tensor."""
    m64, g64, Y, y64 = _gstep_demlin(True)
    m32, g32, _, y32 = _gstep_demlin(False, Y=Y)
    out = {"demlin/g_step": m64, "demlin/g_step_f32": m32, "demlin/Y": Y,
           "demlin/g_forward_dev": np.array(np.abs(y32 - y64).max() / np.abs(y64).max())}
    part = digest_dict("demlin/gradG/", g64)
    out.update(with_dev(part, "demlin/gradG/", g32, G_FLOOR))
    dev = out["demlin/gradG/dev"]
    print("demlin: output range", float(y64.min()), float(y64.max()), "std", float(y64.std()), "g_step", m32, m64, flush=True)
    print("demlin: worst float32-vs-float64 deviation (sample, projection)", dev.max(0), flush=True)
    names = sorted(g32)
    trunk = [i for i, k in enumerate(names) if k.startswith("residual_network/")]
    print("demlin: trunk tensors' worst deviation", dev[trunk].max(0), "others", {k: tuple(float(f"{v:.1e}") for v in dev[i])
                                                                                 for i, k in enumerate(names) if i not in trunk}, flush=True)
    assert dev[trunk].max() < 2.5e-4, "demlin's trunk is meant to be well conditioned"
    return out


if __name__ == "__main__":
    import time

    todo = {"c3": compute_c3, "c3lin": compute_c3lin, "c2": compute_c2, "c5": compute_c5}
    todo_dem = {"dem": compute_dem, "dem5": compute_dem5, "dlin": compute_dlin, "demlin": compute_demlin}  # rounds 3, 4: esrgan_dem
    want = sys.argv[1:] or list(todo)
    for path, table in ((PATH, todo), (PATH_DEM, todo_dem)):
        mine = [n for n in want if n in table]
        if not mine:
            continue
        out = load(path) if (sys.argv[1:] and parts(path)) else {}
        for name in mine:
            t0 = time.time()
            out = {k: v for k, v in out.items() if not k.startswith(name + "/")}
            out.update(table[name]())
            print(name, f"{time.time() - t0:.0f} s", flush=True)
        save(path, out)
        print("wrote", path, [os.path.getsize(p) for p in parts(path)], "bytes")
