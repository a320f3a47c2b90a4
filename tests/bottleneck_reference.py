"""TEST INFRASTRUCTURE: ResNet50 / ResNet101 producers and stride-16 models -- the golden case table, the seeded checkpoints
and images, and the convolution shapes of a Bottleneck block, shared by tests/make_golden_bottleneck.py (runs the unmodified
reference), tests/test_bottleneck_host.py, tests/test_bottleneck_emulated.py and tests/test_gpu_bottleneck.py.

CHECKPOINTS are regenerated from their seed (patch2pix_amd/utils/synthetic.py: make_backbone_checkpoint); a fixture stores the
contrast shift it was made with (a calibration that runs the backbone on the CPU), never weights.

CONVOLUTION BARS.  Default mode: a layer's output may be no farther from the fp64 evaluation than torch's own fp32 convolution
on the same inputs is, times MARGIN = 10, both relative to the image's largest output -- the margin the ResNet34 layer tests
grant (tests/test_kernels_emulated.py: BACKBONE_TOL = 4e-6 against the 4e-7 it records for torch's blocked fp32 convolution;
the emulated MFMA adds its K products one after the other, the worst order there is), and never less than that BACKBONE_TOL
itself at the small K where torch's error is a few units of the last place.  On the CPU build none of the 17 layers needs that
floor: every one passes MARGIN x torch's error alone (kernel / torch: 1.0 ... 9.6, the largest at the 256 -> 256 3x3 layer, K = 2304:
1.85e-6 against 1.92e-7); the floor only keeps the bar from following torch's error below the existing absolute one.  Element-wise on top: the derived bound of
tests/backbone_mode_reference.py (`layer_bound`, K = ci ks^2 from the filter's shape) in both modes; mode 'fp16' is held to that
bound alone."""
import os
from argparse import Namespace

import torch

from patch2pix_amd.utils import synthetic

MARGIN = 10.0
BACKBONE_TOL = 4e-6

# name -> (ci, co, ks, stride, skip, relu): every distinct convolution of a Bottleneck block up to layer3, in its role
# (conv1 / conv2: ReLU; conv3: skip + ReLU; the projection: neither)
LAYERS = {
    "l1_conv1_64_64": (64, 64, 1, 1, False, True),
    "l1_conv2_64_64_3x3": (64, 64, 3, 1, False, True),
    "l1_conv3_64_256": (64, 256, 1, 1, True, True),
    "l1_down_64_256": (64, 256, 1, 1, False, False),
    "l1_conv1_256_64": (256, 64, 1, 1, False, True),
    "l2_conv1_256_128": (256, 128, 1, 1, False, True),
    "l2_conv2_128_128_3x3_s2": (128, 128, 3, 2, False, True),
    "l2_conv3_128_512": (128, 512, 1, 1, True, True),
    "l2_down_256_512_s2": (256, 512, 1, 2, False, False),
    "l2_conv1_512_128": (512, 128, 1, 1, False, True),
    "l3_conv1_512_256": (512, 256, 1, 1, False, True),
    "l3_conv2_256_256_3x3_s2": (256, 256, 3, 2, False, True),
    "l3_conv2_256_256_3x3": (256, 256, 3, 1, False, True),
    "l3_conv3_256_1024": (256, 1024, 1, 1, True, True),
    "l3_down_512_1024_s2": (512, 1024, 1, 2, False, False),
    "l3_down_512_1024": (512, 1024, 1, 1, False, False),
    "l3_conv1_1024_256": (1024, 256, 1, 1, False, True),
}
SIZE = (6, 10)           # two images of 6 x 10: a partial tile in both directions (tiles are 4 or 8 rows of 16 columns)


def layer_inputs(name):
    """Seeded (weight, bn [gamma, beta, mean, var], x [2, ci, 6, 10], skip or None); the images differ by 2^10 in magnitude,
    image 1 has a block of exact zeros (tests/backbone_mode_reference.py: case_inputs, under seeds of this table)."""
    ci, co, ks, stride, skip, _ = LAYERS[name]
    h, w = SIZE
    gen = torch.Generator().manual_seed(7000 + 31 * list(LAYERS).index(name))
    wt = torch.randn(co, ci, ks, ks, generator=gen) * (2.0 / (ci * ks * ks)) ** 0.5
    bn = [torch.rand(co, generator=gen) + 0.5, torch.randn(co, generator=gen) * 0.1, torch.randn(co, generator=gen) * 0.1,
          torch.rand(co, generator=gen) + 0.5]
    x = torch.relu(torch.randn(2, ci, h, w, generator=gen)) * torch.tensor([1.0, 1024.0]).view(2, 1, 1, 1)
    x[1, :, 2:4, 3:7] = 0.0
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    sk = torch.randn(2, co, ho, wo, generator=gen) * x.amax(dim=(1, 2, 3)).view(2, 1, 1, 1) if skip else None
    return wt, bn, x, sk


def check_layer(got, name, mode, what=""):
    """The bars of the module docstring -> (error / bound, error / torch fp32 error), for the records."""
    import backbone_mode_reference as bm
    import torch.nn.functional as F
    wt, bn, x, sk = layer_inputs(name)
    _, _, ks, stride, _, relu = LAYERS[name]
    ref = bm.yardstick(x, wt, bn, stride, sk, relu)
    bound = bm.layer_bound(x.double().abs(), wt, bn, stride, mode, None if sk is None else sk.double().abs())
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert ratio <= 1.0, f"{name} mode {mode}: error {ratio:.3f} of its derived bound"
    # torch's own fp32 evaluation of the same layer
    g, b, m, v = bn
    a = g / torch.sqrt(v + 1e-5)
    y32 = F.conv2d(x, wt, None, stride, ks // 2) * a.view(1, -1, 1, 1) + (b - m * a).view(1, -1, 1, 1)
    if sk is not None:
        y32 = y32 + sk
    y32 = y32.relu() if relu else y32
    scale = ref.abs().amax(dim=(1, 2, 3), keepdim=True)
    e_k, e_t = float((err / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    print(f"{what}{name} mode {mode}: err / bound {ratio:.3f}; err / max |y| kernel {e_k:.2e}, torch fp32 {e_t:.2e}")
    if mode == "fp16x2":
        assert e_k <= max(BACKBONE_TOL, MARGIN * e_t), f"{name}: {e_k:.2e} of the largest output, torch's fp32 convolution {e_t:.2e}"
    return ratio, e_k / max(e_t, 1e-300)


# ---- models ------------------------------------------------------------------------------------------------------------------
SMALL_RC = dict(conv_dims=[64, 64], conv_kers=[3, 3], conv_strs=[2, 1], fc_dims=[64, 32])

# name -> backbone, change_stride, (H1, W1), (H2, W2), ksizes, regressor ('released', 'small' or None), feat_idx, checkpoint seed, image seed
CASES = {
    "bottleneck_r50_s8": ("ResNet50", True, (64, 96), (96, 64), (2,), None, None, 511, 61),     # (seed 501: the reference's own scores 1.04e-5 from fp64)
    "bottleneck_r50_s16": ("ResNet50", False, (128, 192), (128, 192), (2, 1), None, None, 502, 62),
    "bottleneck_r101_s8": ("ResNet101", True, (64, 96), (64, 96), (2,), None, None, 503, 63),
    "bottleneck_r34_s16": ("ResNet34", False, (128, 192), (128, 192), (2,), "released", [0, 1, 2, 3], 504, 64),
    "bottleneck_r50_fi01": ("ResNet50", True, (64, 96), (64, 96), (2,), "small", [0, 1], 505, 65),
}
SCORE_FIXTURE_BAR = 1e-5  # a fixture's recorded scores must be this close to the fp64 ones (tests/make_golden_bottleneck.py)
KAPPA = 1.0              # contrast of the layer-3 features (synthetic.backbone_contrast_shift)


def regressor_config(kind):
    if kind is None:
        return None
    return synthetic.default_regressor_config(**(SMALL_RC if kind == "small" else {}))


def checkpoint(name, contrast):
    """The case's seeded checkpoint; contrast: the stored shift tensor of its fixture, or KAPPA to calibrate (the maker)."""
    backbone, cs, _, _, _, reg, fi, seed, _ = CASES[name]
    return synthetic.make_backbone_checkpoint(seed, backbone, cs, regressor_config(reg), fi, contrast=contrast)


def images(name):
    """[1,3,H,W] fp32 tensors of the case's seeded image pair (normalised as the loaders do)."""
    _, _, (h1, w1), (h2, w2), _, _, _, _, iseed = CASES[name]
    a, b = synthetic.make_image_pair(iseed, max(h1, h2), max(w1, w2))
    return synthetic.image_tensor(a[:h1, :w1].copy())[None], synthetic.image_tensor(b[:h2, :w2].copy())[None]


def model_config(name, ckpt, device):
    backbone, cs, _, _, _, reg, fi, _, _ = CASES[name]
    rc = regressor_config(reg)
    if rc is not None:
        rc.panc = 1
    return Namespace(training=False, device=device, regr_batch=1200, backbone=backbone, feat_idx=fi, weights_dict=ckpt["state_dict"],
                     regressor_config=rc, change_stride=cs)


def sample_channels(t, budget=12288):
    """Every s-th channel of a level [C,h,w] so that at most `budget` values are kept (the fixtures' size) -> (sample, s)."""
    s = max(1, -(-t.numel() // budget))
    return t[::s].contiguous(), s


def golden_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
