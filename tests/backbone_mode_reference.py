"""Backbone mode 'fp16' (P2P_CONV_FP16: one fp16 plane per operand, one MFMA per product in csrc/backbone.hip) -- the case
table, the yardstick, the error bounds and the runners shared by tests/test_backbone_mode_host.py,
tests/test_backbone_mode_emulated.py (the kernel's code on the CPU, tests/hipemu) and tests/test_gpu_backbone_mode.py (MI355X).

YARDSTICK.  Conv2d + folded BatchNorm (eval, eps 1e-5) [+ skip] [+ ReLU] evaluated by torch in fp64 on the CPU from the fp32
inputs, weights and BatchNorm vectors (`yardstick`); for the whole producer the same walk over a ResNet34 module
(`pyramid_yardstick`).

SINGLE-LAYER BOUND, per output element.  u = 2^-24 (fp32), eps = 2^-11 in mode 'fp16'.
  operands    The kernel multiplies every activation of an image by the power of two s that brings the image's largest
              magnitude into [2^11, 2^12) (exact), and every weight of an output channel by the power of two t that does the
              same for the channel (exact, at load time); in mode 'fp16' both are then rounded ONCE to fp16 (round to nearest).
              fp16 is normal from 2^-14 up, i.e. for every value within 2^-25 ... 2^-26 of the maximum: relative error <= eps.
              Below the normal range the spacing is 2^-24 of the scaled unit, so the error is <= 2^-24 ABSOLUTE (scaled).  One
              expression covers both: d(x s) <= max(eps |x s|, 2^-24) for x != 0, and 0 for x = 0 (`operand_error`; the maximum
              is larger than eps |x s| only below 2^-13, where it doubles the normal-range error at most).
  products    x^ w^ - x w = x dw + w dx + dx dw, so the sum of the products is off by at most
              P = sum |x| dw + sum dx |w| + sum dx dw  =  conv(|x| + dx, |w| + dw) - conv(|x|, |w|),
              which is (2 eps + eps^2) sum |x||w| = (2 * 2^-11 + 2^-22) sum |x||w| when every operand is normal.
  accumulate  The products of two fp16 numbers are exact in fp32; K = ci ks ks of them are added in fp32, one after the other
              in the worst case: at most K u relative to the sum of their magnitudes, sum |x^||w^| <= sum |x||w| + P.
  epilogue    fp32: the folded scale a = gamma / sqrt(var + eps_bn) (four roundings and the float eps_bn: <= 5 u), the shift
              beta - mean a (the scale's error and two roundings on |mean a|, one on |beta|), one fused multiply-add, the skip
              addition and the store: every term of  |a| sum |x||w| + |mean a| + |beta| + |skip|  carries less than 10 u.
  bound       |a| (P + K u (sum |x||w| + P)) + 10 u (|a| sum |x||w| + |mean a| + |beta| + |skip|)            (`layer_bound`)
              = (2 * 2^-11 + 2^-22 + K 2^-24) sum |x||w| |a| + the epilogue, in the normal range.
The DEFAULT mode's bound is the same formula with eps = 2^-24, the error of the two-plane split (`EPS` below), and the same
absolute floor (its second plane is subnormal for small operands too).  It is 2^13 times smaller in the operand term; the
accumulation term K u is common to both, so the whole bound is 29 times smaller at K = 576 and 240 times at K = 64.
(2^-24 is the figure csrc/backbone.hip states for its split.  Its strict worst case -- a residual of 13 significant bits
rounded into an 11-bit plane, and the product h1 h1 the kernel drops -- is 2^-22 per term; that excess, 10 u sum |x||w|, is
below the K u term for every layer here, K >= 64, whose own worst case needs every accumulation rounding at its largest with
one sign.)

WHOLE-PYRAMID BOUND.  With e_in the bound on the error of a layer's input, |kernel(x~) - exact(x)| <= |kernel(x~) - exact(x~)| +
|exact(x~) - exact(x)|: the first is the single-layer bound evaluated at |x~| <= |x| + e_in (scale from its maximum, which is
not smaller than the kernel's), the second is linear, |a| conv(e_in, |w|).  A skip adds its own error, ReLU and max-pool are
1-Lipschitz (max-pool: the maximum of the errors in the window), the transposition is exact.  `pyramid_yardstick` evaluates
this next to the fp64 walk.  It is loose (every rounding at its worst with the same sign, through 33 layers); the single-layer
cases carry the weight.  Measured / bound per level is printed by the GPU test and recorded in DESIGN.md section 4.

The tests assert these bounds, never a measured value."""
import ctypes

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
EPS = {"fp16": 2.0 ** -11, "fp16x2": 2.0 ** -24}       # relative operand error per mode
MODE_IDS = {"fp16x2": 0, "fp16": 1}                    # P2P_CONV_FP16X2 / P2P_CONV_FP16 (include/p2p_hip.h)
FLOOR = 2.0 ** -24                                     # absolute operand error below fp16's normal range, in scaled units

# name -> (ci, co, ks, stride, skip, relu): the layer types of layer1 ... layer3 (the 256 -> 256 one walks 8 K chunks through
# the double buffer)
LAYERS = {
    "l1_3x3": (64, 64, 3, 1, False, False),
    "l1_3x3_relu": (64, 64, 3, 1, False, True),
    "l1_3x3_skip": (64, 64, 3, 1, True, False),
    "l1_3x3_skip_relu": (64, 64, 3, 1, True, True),
    "l2_3x3_s2": (64, 128, 3, 2, False, True),
    "l2_down_1x1_s2": (64, 128, 1, 2, False, False),
    "l3_3x3_skip_relu": (256, 256, 3, 1, True, True),
}
SIZES = [(8, 16), (10, 18)]          # exact tiles; partial tiles in both directions (clamped addresses, zero padding at the commit)
CASES = [(name, hw) for name in LAYERS for hw in SIZES]


def case_id(case):
    return f"{case[0]}-{case[1][0]}x{case[1][1]}"


def tiles_of(co):
    """The (mt, nt, wn) tiles csrc/backbone.hip has for a layer of co output channels (conv_cfg)."""
    if co % 256 == 0:
        return [(2, 4, 2), (1, 4, 2), (2, 2, 2), (1, 2, 2)]
    if co % 128 == 0:
        return [(2, 2, 2), (1, 2, 2)]
    return [(1, 2, 1)]


def case_inputs(case):
    """Seeded (weight, bn [gamma, beta, mean, var], x [2, ci, h, w], skip or None) of a case.  The two images differ by 2^10 in
    magnitude (so do their operand scales); image 1 has a block of exact zeros."""
    name, (h, w) = case
    ci, co, ks, stride, skip, _ = LAYERS[name]
    gen = torch.Generator().manual_seed(1000 * list(LAYERS).index(name) + h)
    wt = torch.randn(co, ci, ks, ks, generator=gen) * (2.0 / (ci * ks * ks)) ** 0.5
    bn = [torch.rand(co, generator=gen) + 0.5, torch.randn(co, generator=gen) * 0.1, torch.randn(co, generator=gen) * 0.1,
          torch.rand(co, generator=gen) + 0.5]
    x = torch.relu(torch.randn(2, ci, h, w, generator=gen)) * torch.tensor([1.0, 1024.0]).view(2, 1, 1, 1)
    x[1, :, 2:6, 3:11] = 0.0
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    sk = None
    if skip:
        sk = torch.randn(2, co, ho, wo, generator=gen) * x.amax(dim=(1, 2, 3)).view(2, 1, 1, 1)
    return wt, bn, x, sk


# ---- yardstick and bounds (fp64) ------------------------------------------------------------------------------------------
def _fold(bn):
    g, b, m, v = [t.double() for t in bn]
    a = g / torch.sqrt(v + 1e-5)
    return a, b, m


def pow2_to_top(mx):
    """The exact power of two s with mx s in [2^11, 2^12) (1 for mx = 0): per element of the fp64 tensor mx."""
    _, e = torch.frexp(mx)                        # mx = m 2^e, m in [0.5, 1)
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), 12 - e), torch.ones_like(mx))


def operand_error(t_abs, scale, eps):
    """Bound on |t^ - t| for operands of magnitude t_abs (fp64) rounded under the power-of-two `scale` (broadcastable)."""
    ts = t_abs * scale
    d = torch.maximum(eps * ts, torch.full_like(ts, FLOOR))
    return torch.where(ts == 0, torch.zeros_like(ts), d) / scale


def yardstick(x, wt, bn, stride, skip=None, relu=True):
    a, b, m = _fold(bn)
    y = F.conv2d(x.double(), wt.double(), None, stride, wt.shape[-1] // 2)
    y = y * a.view(1, -1, 1, 1) + (b - m * a).view(1, -1, 1, 1)
    if skip is not None:
        y = y + skip.double()
    return y.relu() if relu else y


def layer_bound(x_abs, wt, bn, stride, mode, skip_abs=None, pad=None):
    """The single-layer bound of the module docstring for inputs of magnitude at most x_abs (fp64 [n, ci, h, w]); per output
    element, fp64."""
    eps = EPS[mode]
    a, b, m = _fold(bn)
    w_abs = wt.double().abs()
    pad = wt.shape[-1] // 2 if pad is None else pad
    dx = operand_error(x_abs, pow2_to_top(x_abs.amax(dim=(1, 2, 3), keepdim=True)), eps)
    dw = operand_error(w_abs, pow2_to_top(w_abs.amax(dim=(1, 2, 3), keepdim=True)), eps)
    s = F.conv2d(x_abs, w_abs, None, stride, pad)
    p = F.conv2d(x_abs + dx, w_abs + dw, None, stride, pad) - s
    k = wt.shape[1] * wt.shape[2] * wt.shape[3]
    aa = a.abs().view(1, -1, 1, 1)
    epi = aa * s + ((m * a).abs() + b.abs()).view(1, -1, 1, 1)
    if skip_abs is not None:
        epi = epi + skip_abs
    return aa * (p + k * U32 * (s + p)) + 10 * U32 * epi


def propagate(e_in, wt, bn, stride, pad=None):
    """|exact(x + e) - exact(x)| <= |a| conv(e_in, |w|)."""
    a, _, _ = _fold(bn)
    pad = wt.shape[-1] // 2 if pad is None else pad
    return F.conv2d(e_in, wt.double().abs(), None, stride, pad) * a.abs().view(1, -1, 1, 1)


def _bn_of(bn):
    return [bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var]


def pyramid_yardstick(extract, image, mode):
    """fp64 walk of the producer (stem, max-pool, the BasicBlocks of layer1 ... layer3 of a float ResNet34 module on the CPU)
    -> (levels [5], bounds [5]): the yardstick pyramid and the propagated error bound of `mode` per element (level 0 is the
    image itself: bound 0)."""
    def step(x, e, conv, bn, skip=None, e_skip=None, relu=True):
        wt, b, st, pad = conv.weight.data, _bn_of(bn), conv.stride[0], conv.padding[0]
        a, beta, mean = _fold(b)
        y = F.conv2d(x, wt.double(), None, st, pad) * a.view(1, -1, 1, 1) + (beta - mean * a).view(1, -1, 1, 1)
        sk_abs = None if skip is None else skip.abs() + e_skip
        eo = layer_bound(x.abs() + e, wt, b, st, mode, sk_abs, pad) + propagate(e, wt, b, st, pad)
        if skip is not None:
            y, eo = y + skip, eo + e_skip
        return (y.relu() if relu else y), eo

    x = image.double()
    e = torch.zeros_like(x)
    levels, bounds = [x], [e]
    x, e = step(x, e, extract.conv1, extract.bn1)
    levels.append(x); bounds.append(e)
    x, e = F.max_pool2d(x, 3, 2, 1), F.max_pool2d(e, 3, 2, 1)
    for name in ("layer1", "layer2", "layer3"):
        for blk in getattr(extract, name):
            skip, e_skip = x, e
            if blk.downsample is not None:
                skip, e_skip = step(x, e, blk.downsample[0], blk.downsample[1], relu=False)
            y, ey = step(x, e, blk.conv1, blk.bn1)
            x, e = step(y, ey, blk.conv2, blk.bn2, skip, e_skip)
        levels.append(x); bounds.append(e)
    return levels, bounds


def check_layer(got, case, mode, what=""):
    """Assert |got - fp64| <= bound element-wise; -> (largest error, largest error / bound) for the records."""
    wt, bn, x, sk = case_inputs(case)
    _, _, _, stride, _, relu = LAYERS[case[0]]
    ref = yardstick(x, wt, bn, stride, sk, relu)
    bound = layer_bound(x.double().abs(), wt, bn, stride, mode, None if sk is None else sk.double().abs())
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}{case_id(case)} mode {mode}: max |err| {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{case_id(case)} mode {mode}: error {ratio:.3f} of its bound"
    return err.max().item(), ratio


# ---- the emulated library (tests/hipemu): the new symbols and a runner ---------------------------------------------------------
def bind(emu):
    """Prototypes of the symbols added in version 112 (tests/hipemu/emu_lib.py copies the ones patch2pix_amd/_lib.py lists)."""
    emu.p2p_conv_set_mode.argtypes, emu.p2p_conv_set_mode.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    emu.p2p_conv_get_mode.argtypes, emu.p2p_conv_get_mode.restype = [ctypes.c_void_p], ctypes.c_int
    emu.p2p_stem_set_mode.argtypes, emu.p2p_stem_set_mode.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    emu.p2p_stem_get_mode.argtypes, emu.p2p_stem_get_mode.restype = [ctypes.c_void_p], ctypes.c_int
    return emu


def emu_conv(emu, wt, bn, stride, x, skip, relu, modes=(), tile=None):
    """p2p_conv_create, p2p_conv_set_mode for every entry of `modes` in turn (none: the handle's mode is never set),
    [p2p_conv_set_tile], p2p_absmax_batch, p2p_conv_forward on CPU tensors (NCHW in and out) -> (y, max |y| per image as the
    kernel reports it)."""
    import emu_lib
    from patch2pix_amd import _lib as real
    co, ci, ks, _ = wt.shape
    keep = [wt.contiguous()] + [t.contiguous() for t in bn]
    b = real.BnParams(*[t.data_ptr() for t in keep[1:]])
    h = ctypes.c_void_p()
    emu_lib.check(emu, emu.p2p_conv_create(emu_lib.ptr(keep[0]), ctypes.byref(b), ci, co, ks, stride, ctypes.byref(h)), "p2p_conv_create")
    try:
        for m in modes:
            emu_lib.check(emu, emu.p2p_conv_set_mode(h, MODE_IDS[m]), "p2p_conv_set_mode")
        assert emu.p2p_conv_get_mode(h) == (MODE_IDS[modes[-1]] if modes else 0)
        if tile:
            emu_lib.check(emu, emu.p2p_conv_set_tile(h, *tile), "p2p_conv_set_tile")
        n, _, hh, ww = x.shape
        xn = x.permute(0, 2, 3, 1).contiguous()
        xmax = torch.zeros(n, dtype=torch.int32)
        emu_lib.check(emu, emu.p2p_absmax_batch(emu_lib.ptr(xn), hh * ww * ci, n, emu_lib.ptr(xmax), None), "p2p_absmax_batch")
        pad = ks // 2
        ho, wo = (hh + 2 * pad - ks) // stride + 1, (ww + 2 * pad - ks) // stride + 1
        y = torch.empty(n, ho, wo, co)
        ymax = torch.zeros(n, dtype=torch.int32)
        res = skip.permute(0, 2, 3, 1).contiguous() if skip is not None else None
        emu_lib.check(emu, emu.p2p_conv_forward(h, emu_lib.ptr(xn), emu_lib.ptr(xmax), n, hh, ww, emu_lib.ptr(res), int(relu),
                                                emu_lib.ptr(y), emu_lib.ptr(ymax), None), "p2p_conv_forward")
    finally:
        emu.p2p_conv_destroy(h)
    return y.permute(0, 3, 1, 2).contiguous(), ymax.view(torch.float32)


def emu_stem(emu, wt, bn, image, mode=None):
    """p2p_stem_create [, p2p_stem_set_mode], p2p_stem_forward on CPU tensors -> level 1 (NCHW)."""
    import emu_lib
    from patch2pix_amd import _lib as real
    keep = [wt.contiguous()] + [t.contiguous() for t in bn]
    b = real.BnParams(*[t.data_ptr() for t in keep[1:]])
    h = ctypes.c_void_p()
    emu_lib.check(emu, emu.p2p_stem_create(emu_lib.ptr(keep[0]), ctypes.byref(b), ctypes.byref(h)), "p2p_stem_create")
    try:
        if mode is not None:
            emu_lib.check(emu, emu.p2p_stem_set_mode(h, MODE_IDS[mode]), "p2p_stem_set_mode")
        image = image.contiguous()
        n, _, hh, ww = image.shape
        imax = torch.zeros(n, dtype=torch.int32)
        emu_lib.check(emu, emu.p2p_absmax_batch(emu_lib.ptr(image), 3 * hh * ww, n, emu_lib.ptr(imax), None), "p2p_absmax_batch")
        y = torch.empty(n, 64, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1)
        emu_lib.check(emu, emu.p2p_stem_forward(h, emu_lib.ptr(image), emu_lib.ptr(imax), n, hh, ww, emu_lib.ptr(y), None), "p2p_stem_forward")
    finally:
        emu.p2p_stem_destroy(h)
    return y


def stem_inputs():
    """Seeded stem weights, BatchNorm vectors and a [2, 3, 21, 70] image batch (partial tiles; image 1 is 2^10 larger and has a
    block of exact zeros)."""
    gen = torch.Generator().manual_seed(77)
    wt = torch.randn(64, 3, 7, 7, generator=gen) * 0.1
    bn = [torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.1, torch.randn(64, generator=gen) * 0.1,
          torch.rand(64, generator=gen) + 0.5]
    image = torch.randn(2, 3, 21, 70, generator=gen) * torch.tensor([1.3, 1.3 * 1024]).view(2, 1, 1, 1)
    image[1, :, 4:12, 9:30] = 0.0
    return wt, bn, image


def check_stem(got, mode, what=""):
    wt, bn, image = stem_inputs()
    ref = yardstick(image, wt, bn, 2, None, True)
    bound = layer_bound(image.double().abs(), wt, bn, 2, mode)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}stem mode {mode}: max |err| {err.max().item():.3e}, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"stem mode {mode}: error {ratio:.3f} of its bound"
    return err.max().item(), ratio
