"""Seeded stress inputs for the regressor kernels: feature pyramids with a wide dynamic range inside one patch and
checkpoints whose weights / BatchNorm parameters leave the one regime `synthetic.make_state_dict` draws from.

The fp16x2 paths carry every fp32 operand of the two convolutions as two fp16 planes under a SHARED power-of-two scale
(one per image patch for the cells of levels 1-3, one per proposal for H = BN1(conv1), one per output channel for the
weights; patch2pix_amd/csrc/regress_h2.hip).  These families put operands far apart under one such scale, or at its
clamp bounds, while the reference's own fp32 evaluation stays within 1e-4 px of fp64 on them.

Plain functions of seeds and sizes; the callers are tests/test_regress_range_emulated.py and
tests/test_gpu_regress_range.py."""
import numpy as np
import torch

from patch2pix_amd.utils import synthetic

LEVEL_DS = (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------------------ pyramids
def _base(seed, H, W):
    return [t.clone() for t in synthetic.make_pyramid(seed, H, W)[:4]]


def region_mask(kind, H, W):
    """bool [H, W] at level-0 resolution, constant on 8 x 8 blocks (= one level-3 cell), so that the four levels of a
    scaled pyramid stay spatially coherent.  'half': the right half; 'checker': a checkerboard of 8-px blocks;
    'corner': the top-left 32 x 32 pixels (larger than a 16-px patch)."""
    by, bx = torch.arange(H)[:, None] // 8, torch.arange(W)[None, :] // 8
    if kind == "half":
        return (bx >= (W // 16)).expand(H, W).clone()
    if kind == "checker":
        return ((by + bx) % 2 == 1)
    if kind == "corner":
        return ((by < 4) & (bx < 4))
    raise ValueError(kind)


def _apply(pyr, mask0, levels, fn):
    for j in levels:
        ds = LEVEL_DS[j]
        m = mask0[::ds, ::ds][:pyr[j].shape[1], :pyr[j].shape[2]]
        pyr[j] = torch.where(m[None], fn(pyr[j]), pyr[j])
    return pyr


def global_scale(seed, H, W, k):
    """Levels 1-3 times 2^k: the exponent clamps of the cell planes (13 / 240) and, at small k, the eps of the norm."""
    pyr = _base(seed, H, W)
    for j in (1, 2, 3):
        pyr[j] = pyr[j] * 2.0 ** k
    return pyr


def contrast(seed, H, W, k, variant="half"):
    """One region ('half' | 'checker') of ALL four levels times 2^k: a pixel's whole 259-vector is scaled, which the
    per-pixel L2 normalisation of the reference undoes exactly -- while a patch across the edge shares one exponent."""
    return contrast_of(_base(seed, H, W), k, variant)


def contrast_of(pyr, k, variant="half"):
    """The same on the first four levels of a pyramid the caller made (a fifth level, which only the coarse stage reads
    and normalises per cell, is kept as it is)."""
    pyr = [t.clone() for t in pyr]
    H, W = pyr[0].shape[1:]
    return _apply(pyr, region_mask(variant, H, W), (0, 1, 2, 3), lambda t: t * 2.0 ** k)


def level_imbalance(seed, H, W, k, level):
    """Only one level (1 or 3) times 2^k: it owns the norm (k > 0) or sits in the low plane of the others (k < 0)."""
    pyr = _base(seed, H, W)
    pyr[level] = pyr[level] * 2.0 ** k
    return pyr


def outlier(seed, H, W, k=12, channel=17, fraction=0.01):
    """One channel of level 2 times 2^k at 1 % of the cells: a single element sets the patch's exponent."""
    pyr = _base(seed, H, W)
    gen = torch.Generator().manual_seed(int(seed) + 104729)
    hit = torch.rand(pyr[2].shape[1:], generator=gen) < fraction
    hit[0, 0] = True                                           # the corner proposal sees one too
    pyr[2][channel] = torch.where(hit, (pyr[2][channel] + 1.0) * 2.0 ** k, pyr[2][channel])
    return pyr


def dead(seed, H, W, level0=False):
    """Levels 1-3 exactly zero in the top-left 32 x 32 pixels; with level0 also level 0 (sum of squares 0, the
    per-pixel scale is 1 / sqrt(1e-6) = 1000, every operand of conv1 is zero there)."""
    return _apply(_base(seed, H, W), region_mask("corner", H, W), (0, 1, 2, 3) if level0 else (1, 2, 3), torch.zeros_like)


def signed(seed, H, W, k=3):
    """Level 0 (the normalised image: not post-ReLU) with large negative values, levels 1-3 non-negative."""
    pyr = _base(seed, H, W)
    pyr[0] = pyr[0] - 3.0 * 2.0 ** k
    return pyr


# --------------------------------------------------------------------------------------------------------- checkpoints
PREFIXES = ("regress_mid.", "regress_fine.")


def _clone(sd):
    return {k: v.clone() for k, v in sd.items()}


def reparam(sd, j, every=3):
    """Channels S = every 3rd of H = BN1(conv1) shrink by 2^j (BN1 weight and bias; running_mean untouched), their
    conv2 input columns grow by 2^j.  No ReLU sits between BN1 and conv2, so the network function is unchanged exactly.
    every=1 shrinks ALL channels: nothing is far below the largest |H| of the proposal, which is itself 2^-j."""
    out = _clone(sd)
    for p in PREFIXES:
        out[p + "conv.1.weight"][::every] *= 2.0 ** -j
        out[p + "conv.1.bias"][::every] *= 2.0 ** -j
        out[p + "conv.2.weight"][:, ::every] *= 2.0 ** j
    return out


def neg_gamma(sd, seed=1):
    """BatchNorm weight negated on a seeded half of the channels of all four BatchNorms of each regressor."""
    out = _clone(sd)
    gen = torch.Generator().manual_seed(seed)
    for p in PREFIXES:
        for name in ("conv.1", "conv.3", "fc.1", "fc.4"):
            w = out[p + name + ".weight"]
            w[torch.rand(w.shape[0], generator=gen) < 0.5] *= -1.0
    return out


def var_spread(sd, seed=2):
    """running_var of BN1 / BN2 log-uniform in [1e-4, 1e2]: folded scales over three decades each way."""
    out = _clone(sd)
    gen = torch.Generator().manual_seed(seed)
    for p in PREFIXES:
        for name in ("conv.1", "conv.3"):
            out[p + name + ".running_var"] = 10.0 ** (torch.rand(512, generator=gen) * 6.0 - 4.0)
    return out


def dead_channels(sd, seed=3):
    """8 output channels of conv1 and of conv2 all-zero, plus 8 input columns of conv2 zero."""
    out = _clone(sd)
    gen = torch.Generator().manual_seed(seed)
    for p in PREFIXES:
        out[p + "conv.0.weight"][torch.randperm(512, generator=gen)[:8]] = 0.0
        out[p + "conv.2.weight"][torch.randperm(512, generator=gen)[:8]] = 0.0
        out[p + "conv.2.weight"][:, torch.randperm(512, generator=gen)[:8]] = 0.0
    return out


def octaves(sd, seed=4):
    """Per-output-channel magnitudes of conv1 / conv2 times 2^U(-9..3) (the spread of _seeded_conv_weights), undone in
    the BatchNorm that follows (weight / s, running_mean * s): the network function is unchanged exactly."""
    out = _clone(sd)
    rng = np.random.default_rng(seed)
    for p in PREFIXES:
        for conv, bn in (("conv.0", "conv.1"), ("conv.2", "conv.3")):
            s = torch.from_numpy(np.exp2(rng.integers(-9, 4, 512)).astype(np.float32))
            out[p + conv + ".weight"] *= s.view(-1, 1, 1, 1)
            out[p + bn + ".weight"] /= s
            out[p + bn + ".running_mean"] *= s
    return out


RAW_TARGET = (0.45, 0.5, 0.55, 0.4, 0.2)       # the centre synthetic._regressor calibrates the five raw outputs to


def recentre(sd, prefix, raw_mean):
    """fc.6.bias += RAW_TARGET - raw_mean (in place): `raw_mean` is the mean over the caller's proposals of the fp64
    reference's five raw outputs of this regressor, as synthetic._regressor does on its pilot patches."""
    sd[prefix + "fc.6.bias"] += (torch.tensor(RAW_TARGET, dtype=torch.float64) - raw_mean.double()).float()


def calm(sd, prefix, raw_std, target=0.25):
    """Rows of fc.6.weight (and fc.6.bias) scaled DOWN so that no raw output spreads more than `target` over the caller's
    proposals (in place; `raw_std`: the fp64 reference's standard deviation per output).  var_spread amplifies single
    channels a hundredfold: un-calmed, the raw outputs spread over +-300 and every coordinate sits on a clamp bound,
    whatever the bias.  The convolutions, whose folded scales the family is about, are not touched."""
    f = torch.clamp(target / raw_std.double().clamp_min(1e-30), max=1.0).float()
    sd[prefix + "fc.6.weight"] *= f.view(5, 1)
    sd[prefix + "fc.6.bias"] *= f


def _seeded_conv_weights():
    """conv1 / conv2 weights of a regressor with per-channel magnitudes over 13 octaves and one channel of zeros each."""
    rng = np.random.default_rng(20261016)
    out = []
    for cin in (518, 512):
        w = rng.standard_normal((512, cin, 3, 3)).astype(np.float32)
        w *= np.exp2(rng.integers(-9, 4, (512, 1, 1, 1))).astype(np.float32)
        out.append(w)
    out[0][7] = 0.0
    out[1][300] = 0.0
    return out
