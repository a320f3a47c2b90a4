"""Torch-tensor front end of the C ABI: owns nothing but the two kinds of weight handle.
Every function launches asynchronously on torch's current HIP stream of the tensors' device."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib, staging


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name} must be a float32 tensor on the GPU (got {t.dtype}, {t.device})")
    return t.contiguous()


def _host(t):
    return t.detach().to("cpu", torch.float32).contiguous()


RELEASED_NCN_LAYOUT = dict(kernel_sizes=[3, 3], channels=[16, 1], symmetric_mode=True)
NCN_MAX_LAYERS, NCN_KERNEL_SIZES, NCN_MAX_CHANNELS = 4, (3, 5), 16       # include/p2p_hip.h, p2p_ncn_config


def ncn_layout(source=None, symmetric_mode=None):
    """The NeighConsensus stack (reference networks/ncn/model.py:124-143) a checkpoint or a configuration describes, as
    dict(kernel_sizes, channels, symmetric_mode) of plain lists, checked against what the library implements.  `source`:
    a sub-state_dict ('conv.{2i}.weight' in the stored layout [k, c_out, c_in, k, k, k], conv4d.py:119-120) whose shapes
    are read, a namespace or dict with kernel_sizes / channels (/ symmetric_mode), or None (the released stack).  A stack
    the reference accepts and the library does not raises NotImplementedError, a malformed one ValueError; no GPU needed."""
    if source is None:
        lay = {k: (list(v) if isinstance(v, list) else v) for k, v in RELEASED_NCN_LAYOUT.items()}
    elif isinstance(source, dict) and any(str(k).startswith("conv.") for k in source):
        ks, ch, cin, i = [], [], 1, 0
        while f"conv.{2 * i}.weight" in source:
            shp = tuple(source[f"conv.{2 * i}.weight"].shape)
            if len(shp) != 6 or len({shp[0], shp[3], shp[4], shp[5]}) != 1:
                raise ValueError(f"conv.{2 * i}.weight has shape {shp}: expected the stored layout [k, c_out, c_in, k, k, k]")
            if shp[2] != cin:
                raise ValueError(f"conv.{2 * i}.weight has {shp[2]} input channels where the layer below it gives {cin}")
            bias = source.get(f"conv.{2 * i}.bias")
            if bias is None or tuple(bias.shape) != (shp[1],):
                raise ValueError(f"conv.{2 * i}.bias is missing or is not of shape ({shp[1]},)")
            ks.append(int(shp[0])); ch.append(int(shp[1])); cin = shp[1]; i += 1
        if not ks:
            raise ValueError("no conv.0.weight among the consensus tensors")
        lay = dict(kernel_sizes=ks, channels=ch, symmetric_mode=True)
    else:
        get = (lambda k, d=None: source.get(k, d)) if isinstance(source, dict) else (lambda k, d=None: getattr(source, k, d))
        ks, ch = get("kernel_sizes"), get("channels")
        if ks is None or ch is None:
            raise ValueError("a consensus configuration needs kernel_sizes and channels")
        lay = dict(kernel_sizes=[int(k) for k in ks], channels=[int(c) for c in ch], symmetric_mode=bool(get("symmetric_mode", True)))
    if symmetric_mode is not None:
        lay["symmetric_mode"] = bool(symmetric_mode)
    ks, ch = lay["kernel_sizes"], lay["channels"]
    if not ks or len(ks) != len(ch):
        raise ValueError(f"kernel_sizes {ks} and channels {ch} must be non-empty lists of one length")
    if any(k <= 0 for k in ks) or any(c <= 0 for c in ch):
        raise ValueError(f"kernel_sizes {ks} / channels {ch}: sizes must be positive")
    if len(ks) > NCN_MAX_LAYERS:
        raise NotImplementedError(f"kernel_sizes {ks}: at most {NCN_MAX_LAYERS} consensus layers are implemented")
    if any(k not in NCN_KERNEL_SIZES for k in ks):
        raise NotImplementedError(f"kernel_sizes {ks}: kernel sizes 3 and 5 are implemented")
    if any(c > NCN_MAX_CHANNELS for c in ch):
        raise NotImplementedError(f"channels {ch}: at most {NCN_MAX_CHANNELS} channels per layer are implemented")
    if ch[-1] != 1:
        raise NotImplementedError(f"channels {ch}: the last layer must have one channel (the volume is [B,1,...] downstream)")
    return lay


def ncn_shapes(lay):
    """State_dict keys -> shapes of the NeighConsensus of an `ncn_layout` in the stored layout (conv4d.py:119-120)."""
    shapes, cin = {}, 1
    for i, (k, c) in enumerate(zip(lay["kernel_sizes"], lay["channels"])):
        shapes[f"conv.{2 * i}.weight"], shapes[f"conv.{2 * i}.bias"] = (k, c, cin, k, k, k), (c,)
        cin = c
    return shapes


def coarse_mode_id(mode):
    """'fp16x2' | 'fp16' -> P2P_COARSE_FP16X2 | P2P_COARSE_FP16 (include/p2p_hip.h); anything else raises ValueError."""
    if not isinstance(mode, str) or mode not in _lib.COARSE_MODES:
        raise ValueError(f"unknown coarse mode {mode!r}: one of {sorted(_lib.COARSE_MODES)}")
    return _lib.COARSE_MODES[mode]


def default_coarse_mode():
    """The mode new tuned NcnWeights handles start in: P2P_COARSE_MODE=fp16x2|fp16 (tools; read here, not in the library)."""
    return os.environ.get("P2P_COARSE_MODE") or "fp16x2"


def default_coarse_generic_mode():
    """The mode new generic NcnWeights handles start in: P2P_COARSE_GENERIC_MODE=generic|generic_fp16x2 (read here, not in the
    library); P2P_COARSE_MODE applies to tuned handles only."""
    return os.environ.get("P2P_COARSE_GENERIC_MODE") or "generic"


class NcnWeights:
    """Device-resident NeighConsensus filters (reference networks/ncn/model.py:124-143).  The constructor takes the released
    stack's four tensors (the tuned kernel); `from_state_dict` takes any stack within `ncn_layout`'s limits."""

    layout, generic = RELEASED_NCN_LAYOUT, False

    def __init__(self, w1, b1, w2, b2, device):
        keep = [_host(w1), _host(b1), _host(w2), _host(b2)]
        if tuple(keep[0].shape) != (3, 16, 1, 3, 3, 3) or tuple(keep[2].shape) != (3, 1, 16, 3, 3, 3):
            raise NotImplementedError("only NeighConsensus(kernel_sizes=[3,3], channels=[16,1]) is implemented")
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_ncn_create(*[t.data_ptr() for t in keep], ctypes.byref(self.handle)), "p2p_ncn_create")
        self.device = torch.device(device)
        if default_coarse_mode() != "fp16x2":
            self.set_mode(default_coarse_mode())

    @classmethod
    def from_state_dict(cls, sd, device, symmetric_mode=True, generic=False):
        """`sd`: the sub-state_dict of the consensus net ('conv.0.weight', 'conv.0.bias', 'conv.2.weight', ...).  The released
        stack with symmetric_mode and without `generic` runs the tuned kernel; every other one -- or `generic=True` -- a
        generic handle (p2p_ncn_create_config: exact fp32 MFMA, one launch per layer and branch)."""
        lay = ncn_layout({k: v for k, v in sd.items() if k.startswith("conv.")}, symmetric_mode)
        if not generic and lay == RELEASED_NCN_LAYOUT:
            return cls(sd["conv.0.weight"], sd["conv.0.bias"], sd["conv.2.weight"], sd["conv.2.bias"], device)
        n = len(lay["kernel_sizes"])
        keep = [(_host(sd[f"conv.{2 * i}.weight"]), _host(sd[f"conv.{2 * i}.bias"])) for i in range(n)]
        c, t = _lib.NcnConfig(), _lib.NcnTensors()
        c.n_layers, c.symmetric = n, int(lay["symmetric_mode"])
        for i in range(n):
            c.kernel_size[i], c.channels[i] = lay["kernel_sizes"][i], lay["channels"][i]
            t.w[i], t.b[i] = keep[i][0].data_ptr(), keep[i][1].data_ptr()
        self = cls.__new__(cls)
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_ncn_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(self.handle)), "p2p_ncn_create_config")
        self.device, self.layout, self.generic = torch.device(device), lay, True
        if default_coarse_generic_mode() != "generic":
            self.set_mode(default_coarse_generic_mode())
        return self

    def set_tile(self, ta=0, tb=0, tc=0):
        """Force the work-group tile of the consensus kernel (tests, sweeps); (0, 0, 0) = automatic.  Results do not depend on it."""
        if self.generic:
            raise NotImplementedError("set_tile: a generic consensus handle has no work-group tile to force")
        _lib.check(_lib.p2p_ncn_set_tile(self.handle, int(ta), int(tb), int(tc)), "p2p_ncn_set_tile")

    def set_mode(self, mode):
        """'fp16x2' (default: fp32-equivalent, two fp16 planes per operand, 3 MFMA products) or the opt-in 'fp16': the matrix-core
        kernels of every coarse-stage call with this handle (feature preparation, correlation + pooling, the fused consensus
        kernel) run with ONE fp16 plane per operand and one MFMA product -- relative operand rounding 2^-11, NOT
        fp32-equivalent ("Single-plane mode of the coarse stage").  Nothing is packed or uploaded.
        A generic handle has names of its own: 'generic' (default, exact fp32 MFMA) and the opt-in 'generic_fp16x2' (every layer
        behind the first on the fp16 matrix cores, two fp16 planes per operand, three MFMA products: fp32-equivalent; the planes are
        packed and uploaded on the first selection; DESIGN.md section 4, "fp16x2 mode of the generic consensus net").  A name of the
        other kind of handle raises NotImplementedError, an unknown one ValueError, both before the library is asked."""
        names = _lib.COARSE_MODES_GENERIC if self.generic else _lib.COARSE_MODES
        if not isinstance(mode, str) or (mode not in _lib.COARSE_MODES and mode not in _lib.COARSE_MODES_GENERIC):
            raise ValueError(f"unknown coarse mode {mode!r}: one of {sorted(names)}")
        if mode not in names:
            raise NotImplementedError(f"set_mode: {mode!r} is no mode of a {'generic' if self.generic else 'tuned'} consensus handle "
                                      f"(one of {sorted(names)})")
        with torch.cuda.device(self.device):                        # (the first selection of 'generic_fp16x2' uploads)
            _lib.check(_lib.p2p_ncn_set_mode(self.handle, names[mode]), "p2p_ncn_set_mode")

    @property
    def mode(self):
        mid = _lib.p2p_ncn_get_mode(self.handle)
        if self.generic and mid:
            return next(k for k, v in _lib.COARSE_MODES_GENERIC.items() if v == mid)
        return next(k for k, v in _lib.COARSE_MODES.items() if v == mid)

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:      # _lib is None during interpreter shutdown
            _lib.p2p_ncn_destroy(self.handle)
            self.handle = None


# Experiments and the tile-independence tests: (mt, nt, wn) forced on every ConvBN launch (p2p_conv_set_tile); None = the
# library picks by launch size.  The environment variable P2P_CONV_TILE="mt,nt,wn" sets it at import (tools).
def _parse_conv_tile(text):
    try:
        t = tuple(int(v) for v in text.split(","))
    except ValueError:
        t = ()
    if len(t) != 3 or min(t) < 0:
        raise ValueError(f"P2P_CONV_TILE={text!r}: expected three non-negative integers 'mt,nt,wn'")
    return t


FORCED_CONV_TILE = _parse_conv_tile(os.environ["P2P_CONV_TILE"]) if os.environ.get("P2P_CONV_TILE") else None


def backbone_mode_id(mode):
    """'fp16x2' | 'fp16' -> P2P_CONV_FP16X2 | P2P_CONV_FP16 (include/p2p_hip.h); anything else raises ValueError."""
    if mode not in _lib.BACKBONE_MODES:
        raise ValueError(f"unknown backbone mode {mode!r}: one of {sorted(_lib.BACKBONE_MODES)}")
    return _lib.BACKBONE_MODES[mode]


def default_backbone_mode():
    """The mode new ConvBN / Stem handles start in: P2P_BACKBONE_MODE=fp16x2|fp16 (tools; read here, not in the library)."""
    return os.environ.get("P2P_BACKBONE_MODE") or "fp16x2"


class _BackboneMode:
    """set_mode / mode of the two handle kinds of the pyramid producer (`_set_mode` / `_get_mode`: the handle kind's setter
    and getter of the C ABI)."""

    def set_mode(self, mode):
        """'fp16x2' (default: fp32-equivalent, two fp16 planes per operand under exact power-of-two scales, 3 MFMA products)
        or the opt-in 'fp16' (the same kernel with ONE plane per operand and one MFMA product: relative operand rounding
        2^-11, NOT fp32-equivalent; DESIGN.md section 4, "Single-plane mode of the producer").  Both read the one packed weight
        blob: nothing is packed or uploaded."""
        _lib.check(self._set_mode(self.handle, backbone_mode_id(mode)), self._set_mode.__name__)

    @property
    def mode(self):
        mid = self._get_mode(self.handle)
        return next(k for k, v in _lib.BACKBONE_MODES.items() if v == mid)


class ConvBN(_BackboneMode):
    """Device-resident packed Conv2d(bias=False) + BatchNorm2d (eval) of the pyramid producer
    (reference networks/resnet.py:26-60); `forward` works on fp32 NHWC activations."""
    _set_mode, _get_mode = staticmethod(_lib.p2p_conv_set_mode), staticmethod(_lib.p2p_conv_get_mode)

    def __init__(self, conv_weight, bn_weight, bn_bias, bn_mean, bn_var, stride, device):
        keep = [_host(t) for t in (conv_weight, bn_weight, bn_bias, bn_mean, bn_var)]
        co, ci, ks, ks2 = keep[0].shape
        if ks != ks2:
            raise NotImplementedError("square kernels only")
        bn = _lib.BnParams(*[t.data_ptr() for t in keep[1:]])
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_conv_create(keep[0].data_ptr(), ctypes.byref(bn), ci, co, ks, int(stride), ctypes.byref(self.handle)),
                       "p2p_conv_create")
        self.ci, self.co, self.ks, self.stride = ci, co, ks, int(stride)
        self.device = torch.device(device)
        self._tile = None
        if default_backbone_mode() != "fp16x2":
            self.set_mode(default_backbone_mode())

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.p2p_conv_destroy(self.handle)
            self.handle = None

    def forward(self, x, xmax, residual=None, relu=True, ymax=None):
        """x [n,h,w,ci] fp32 NHWC, xmax [n] int32 (float bits of max |x| per image) -> y [n,ho,wo,co]; ymax (optional
        [n] int32, ZERO on entry) receives the float bits of max |y| per image."""
        n, h, w, ci = x.shape
        if ci != self.ci or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise TypeError(f"ConvBN.forward: expected a contiguous float32 NHWC tensor with {self.ci} channels on the GPU")
        if FORCED_CONV_TILE != self._tile:
            _lib.check(_lib.p2p_conv_set_tile(self.handle, *(FORCED_CONV_TILE or (0, 0, 0))), "p2p_conv_set_tile")
            self._tile = FORCED_CONV_TILE
        pad = self.ks // 2
        ho, wo = (h + 2 * pad - self.ks) // self.stride + 1, (w + 2 * pad - self.ks) // self.stride + 1
        y = torch.empty((n, ho, wo, self.co), device=x.device, dtype=torch.float32)
        if residual is not None and (residual.shape != y.shape or not residual.is_contiguous()):
            raise TypeError("ConvBN.forward: residual must be a contiguous NHWC tensor of the output's shape")
        _lib.check(_lib.p2p_conv_forward(self.handle, x.data_ptr(), xmax.data_ptr(), n, h, w,
                                         residual.data_ptr() if residual is not None else None, int(relu), y.data_ptr(),
                                         ymax.data_ptr() if ymax is not None else None, _stream()), "p2p_conv_forward")
        return y


class Stem(_BackboneMode):
    """Device-resident packed conv1 7x7/2 + bn1 (+ ReLU) of the pyramid producer (reference networks/resnet.py:101-103)."""
    _set_mode, _get_mode = staticmethod(_lib.p2p_stem_set_mode), staticmethod(_lib.p2p_stem_get_mode)

    def __init__(self, conv_weight, bn_weight, bn_bias, bn_mean, bn_var, device):
        keep = [_host(t) for t in (conv_weight, bn_weight, bn_bias, bn_mean, bn_var)]
        if tuple(keep[0].shape) != (64, 3, 7, 7):
            raise NotImplementedError("only the ResNet stem Conv2d(3, 64, 7, 2, 3) is implemented")
        bn = _lib.BnParams(*[t.data_ptr() for t in keep[1:]])
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_stem_create(keep[0].data_ptr(), ctypes.byref(bn), ctypes.byref(self.handle)), "p2p_stem_create")
        self.device = torch.device(device)
        if default_backbone_mode() != "fp16x2":
            self.set_mode(default_backbone_mode())

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.p2p_stem_destroy(self.handle)
            self.handle = None

    def forward(self, image):
        """image [n,3,h,w] fp32 NCHW -> relu(bn1(conv1(image))) [n,64,ho,wo] NCHW."""
        image = _f32c(image, "image")
        n, c, h, w = image.shape
        if c != 3:
            raise TypeError("Stem.forward: three-channel images only")
        imax = absmax_batch(image)
        y = torch.empty((n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1), device=image.device, dtype=torch.float32)
        _lib.check(_lib.p2p_stem_forward(self.handle, image.data_ptr(), imax.data_ptr(), n, h, w, y.data_ptr(), _stream()), "p2p_stem_forward")
        return y


def maxpool_nhwc(x, ymax=None):
    """MaxPool2d(3, 2, 1) of x [n,c,h,w] NCHW -> y [n,hp,wp,c] NHWC; ymax: optional [n] int32, ZERO on entry."""
    x = _f32c(x, "x")
    n, c, h, w = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=x.device, dtype=torch.float32)
    _lib.check(_lib.p2p_maxpool_nhwc(x.data_ptr(), n, c, h, w, y.data_ptr(), ymax.data_ptr() if ymax is not None else None, _stream()),
               "p2p_maxpool_nhwc")
    return y


def nhwc_to_nchw(x):
    """x [n,h,w,c] -> [n,c,h,w] contiguous."""
    x = _f32c(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    _lib.check(_lib.p2p_nhwc_to_nchw(x.data_ptr(), n, h, w, c, y.data_ptr(), _stream()), "p2p_nhwc_to_nchw")
    return y


def absmax_batch(x):
    """x [n, ...] contiguous fp32 on the GPU -> [n] int32: float bits of max |x| per item."""
    x = _f32c(x, "x")
    out = torch.empty((x.shape[0],), device=x.device, dtype=torch.int32)
    _lib.check(_lib.p2p_absmax_batch(x.data_ptr(), x[0].numel(), x.shape[0], out.data_ptr(), _stream()), "p2p_absmax_batch")
    return out


FEAT_DIMS = (3, 64, 64, 128, 256)          # channels of the pyramid levels (networks/resnet.py:138-157)
RELEASED_LAYOUT = dict(feat_idx=[0, 1, 2, 3], feat_comb="pre", conv_dims=[512, 512], conv_kers=[3, 3], conv_strs=[2, 1],
                       fc_dims=[512, 256], psize=[16, 16])


def regressor_layout(config=None, feat_idx=None):
    """The regressor a checkpoint describes (`regressor_config` namespace or dict + `feat_idx`; None = the released one),
    normalised and checked against what the library implements (include/p2p_hip.h, p2p_regressor_config): a dict
    feat_idx / feat_comb / conv_dims / conv_kers / conv_strs / fc_dims / psize of plain lists.  A configuration the
    reference accepts and the library does not raises NotImplementedError, a malformed one ValueError; no GPU needed."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    lay = {k: (list(v) if isinstance(v, list) else v) for k, v in RELEASED_LAYOUT.items()}
    if feat_idx is not None:
        lay["feat_idx"] = [int(i) for i in feat_idx]
    if config is not None:
        lay["feat_comb"] = get("feat_comb", "pre")
        lay["conv_dims"] = [int(d) for d in get("conv_dims")]
        lay["conv_kers"] = [int(k) for k in get("conv_kers")]
        strs = get("conv_strs")                      # absent: [2] * len(conv_kers) (networks/modules.py:60)
        lay["conv_strs"] = [int(v) for v in strs] if strs is not None else [2] * len(lay["conv_kers"])
        lay["fc_dims"] = [int(d) for d in get("fc_dims")]
        ps = get("psize", [16, 16])
        lay["psize"] = [int(v) for v in ps] if isinstance(ps, (list, tuple)) else [int(ps), int(ps)]
    fi = lay["feat_idx"]
    if not fi or any(b <= a for a, b in zip(fi, fi[1:])) or any(i < 0 or i > 4 for i in fi):
        raise ValueError(f"feat_idx {fi}: a non-empty, strictly ascending list of pyramid levels")
    if 4 in fi:
        raise NotImplementedError(f"feat_idx {fi}: level 4 is not implemented by the fine stage (the pyramid handed to the "
                                  "library carries levels 0..3)")
    if lay["psize"] != [16, 16]:
        raise NotImplementedError(f"psize {lay['psize']}: psize must be [16,16]")
    if lay["feat_comb"] not in ("pre", "post"):
        raise ValueError(f"feat_comb {lay['feat_comb']!r}: 'pre' or 'post'")
    nc = len(lay["conv_dims"])
    if nc == 0 or len(lay["conv_kers"]) != nc or len(lay["conv_strs"]) != nc:
        raise ValueError("conv_dims, conv_kers and conv_strs must be non-empty lists of one length")
    if nc > 4 or len(lay["fc_dims"]) > 4:
        raise NotImplementedError("at most 4 convolutions and 4 hidden FC layers are implemented")
    for what in ("conv_dims", "fc_dims"):
        for d in lay[what]:
            if d <= 0:
                raise ValueError(f"{what} {lay[what]}: dims must be positive")
            if d % 16 or d > 1024:
                raise NotImplementedError(f"{what} {lay[what]}: dims must be multiples of 16 in [16, 1024]")
    side = 16
    for k, st in zip(lay["conv_kers"], lay["conv_strs"]):
        if k not in (1, 3, 5):
            raise NotImplementedError(f"conv_kers {lay['conv_kers']}: kernel sizes 1, 3 and 5 are implemented")
        if st not in (1, 2):
            raise NotImplementedError(f"conv_strs {lay['conv_strs']}: strides 1 and 2 are implemented")
        if side + 2 - k < 0:
            raise ValueError(f"conv_kers {lay['conv_kers']} / conv_strs {lay['conv_strs']}: the map shrinks below 1x1")
        side = (side + 2 - k) // st + 1
    return lay


def regressor_shapes(lay):
    """State_dict keys -> shapes of the FeatRegressNet of a `regressor_layout` (weights and biases; BatchNorm vectors are
    listed as 'conv.1' -> n, 'fc.1' -> n under 'bn'), as the reference module builds them (networks/modules.py:76-99)."""
    feat_dim = sum(FEAT_DIMS[i] for i in lay["feat_idx"])
    cin = feat_dim if lay["feat_comb"] == "post" else 2 * feat_dim
    shapes, bns = {}, {}
    for i, (d, k) in enumerate(zip(lay["conv_dims"], lay["conv_kers"])):
        shapes[f"conv.{2 * i}.weight"] = (d, cin, k, k)
        bns[f"conv.{2 * i + 1}"] = d
        cin = d
    k = lay["conv_dims"][-1] * (2 if lay["feat_comb"] == "post" else 1)
    for i, d in enumerate(lay["fc_dims"]):
        shapes[f"fc.{3 * i}.weight"], shapes[f"fc.{3 * i}.bias"] = (d, k), (d,)
        bns[f"fc.{3 * i + 1}"] = d
        k = d
    n = 3 * len(lay["fc_dims"])
    shapes[f"fc.{n}.weight"], shapes[f"fc.{n}.bias"] = (5, k), (5,)
    return shapes, bns


class RegressorWeights:
    """Device-resident packed FeatRegressNet (reference networks/modules.py:56-112).
    `sd` maps the sub-state_dict keys ('conv.0.weight', 'fc.6.bias', ...) to tensors.  `config` / `feat_idx`: the
    checkpoint's `regressor_config` / `feat_idx` (None = the released ones).  The released configuration runs the tuned
    kernels; every other one -- or `generic=True` -- a generic handle (p2p_regressor_create_config: one launch per layer; exact
    fp32 MFMA by default, `set_mode("generic_fp16x2")` or P2P_REGRESS_GENERIC_MODE for the fp16x2 convolution stack)."""

    def __init__(self, sd, device, config=None, feat_idx=None, generic=False):
        lay = regressor_layout(config, feat_idx)
        self.layout = lay
        self.generic = bool(generic) or lay != RELEASED_LAYOUT
        self.device = torch.device(device)
        if self.generic:
            self._create_generic(sd, lay)
            return
        exp = {"conv.0.weight": (512, 518, 3, 3), "conv.2.weight": (512, 512, 3, 3), "fc.0.weight": (512, 512),
               "fc.3.weight": (256, 512), "fc.6.weight": (5, 256)}
        for k, shp in exp.items():
            if tuple(sd[k].shape) != shp:
                raise NotImplementedError(f"regressor {k} has shape {tuple(sd[k].shape)}; only the released "
                                          f"configuration {shp} is implemented")
        keep = {k: _host(v) for k, v in sd.items() if v.is_floating_point()}
        p = _lib.RegressorParams()

        def bn(prefix):
            return _lib.BnParams(keep[prefix + ".weight"].data_ptr(), keep[prefix + ".bias"].data_ptr(),
                                 keep[prefix + ".running_mean"].data_ptr(), keep[prefix + ".running_var"].data_ptr())

        p.conv1_w = keep["conv.0.weight"].data_ptr(); p.bn1 = bn("conv.1")
        p.conv2_w = keep["conv.2.weight"].data_ptr(); p.bn2 = bn("conv.3")
        p.fc1_w = keep["fc.0.weight"].data_ptr(); p.fc1_b = keep["fc.0.bias"].data_ptr(); p.bnf1 = bn("fc.1")
        p.fc2_w = keep["fc.3.weight"].data_ptr(); p.fc2_b = keep["fc.3.bias"].data_ptr(); p.bnf2 = bn("fc.4")
        p.fc3_w = keep["fc.6.weight"].data_ptr(); p.fc3_b = keep["fc.6.bias"].data_ptr()
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_regressor_create(ctypes.byref(p), ctypes.byref(self.handle)), "p2p_regressor_create")
        env = os.environ.get("P2P_REGRESS_MODE")       # tools: the mode new handles start in (read here, not in the library)
        if env:
            self.set_mode(env)

    def _create_generic(self, sd, lay):
        shapes, bns = regressor_shapes(lay)
        for k, shp in shapes.items():
            if k not in sd or tuple(sd[k].shape) != shp:
                got = tuple(sd[k].shape) if k in sd else "no tensor"
                raise ValueError(f"regressor {k}: the configuration asks for shape {shp}, the state_dict has {got}")
        keep = {k: _host(v) for k, v in sd.items() if v.is_floating_point()}

        def bn(prefix):
            return _lib.BnParams(keep[prefix + ".weight"].data_ptr(), keep[prefix + ".bias"].data_ptr(),
                                 keep[prefix + ".running_mean"].data_ptr(), keep[prefix + ".running_var"].data_ptr())

        c, t = _lib.RegressorConfig(), _lib.RegressorTensors()
        c.n_feat = len(lay["feat_idx"])
        for i, j in enumerate(lay["feat_idx"]):
            c.feat_idx[i] = j
        c.feat_comb = _lib.FEAT_COMB[lay["feat_comb"]]
        c.n_conv, c.n_fc, c.psize = len(lay["conv_dims"]), len(lay["fc_dims"]), lay["psize"][0]
        for i in range(c.n_conv):
            c.conv_dim[i], c.conv_ker[i], c.conv_str[i] = lay["conv_dims"][i], lay["conv_kers"][i], lay["conv_strs"][i]
            t.conv_w[i] = keep[f"conv.{2 * i}.weight"].data_ptr()
            t.conv_bn[i] = bn(f"conv.{2 * i + 1}")
        for i in range(c.n_fc):
            c.fc_dim[i] = lay["fc_dims"][i]
            t.fc_w[i], t.fc_b[i] = keep[f"fc.{3 * i}.weight"].data_ptr(), keep[f"fc.{3 * i}.bias"].data_ptr()
            t.fc_bn[i] = bn(f"fc.{3 * i + 1}")
        t.out_w, t.out_b = keep[f"fc.{3 * c.n_fc}.weight"].data_ptr(), keep[f"fc.{3 * c.n_fc}.bias"].data_ptr()
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.p2p_regressor_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(self.handle)),
                       "p2p_regressor_create_config")
        env = os.environ.get("P2P_REGRESS_GENERIC_MODE")      # tools: the mode new GENERIC handles start in (read here, not in the library)
        if env:
            self.set_mode(env)

    def set_mode(self, mode):
        """'fp16x2w' (default: fp32-equivalent, two fp16 planes under exact power-of-two scales, 3 MFMA products, the second
        convolution as Winograd F(2x2,3x3) GEMMs), 'fp16x2' (the same arithmetic, both convolutions direct, one launch) or 'f32'
        (exact fp32 MFMA) -- all three fp32-equivalent -- or the opt-in 'fp16' (the structure of 'fp16x2w' with ONE fp16 plane per
        operand and one MFMA product: relative operand rounding 2^-11, NOT held to the 1e-3 px / 1e-5 bars of the others;
        DESIGN.md section 4, "Single-plane mode").  The first selection of a
        non-default mode packs and uploads that mode's weight stream (host work, ~1 s)."""
        modes = {**_lib.REGRESS_MODES, **_lib.REGRESS_MODES_LOSSY}
        if self.generic:
            # 'generic' (default: exact fp32 MFMA) or the opt-in 'generic_fp16x2' (the convolution stack on two fp16 planes per
            # operand, three MFMA products, fp32-equivalent: DESIGN.md section 4, "The generic regressor"); the first selection of
            # the latter packs and uploads its weight planes, going back gives the earlier outputs bit for bit
            if mode in modes:
                raise NotImplementedError(f"regressor mode {mode!r}: a generic regressor runs one of {sorted(_lib.REGRESS_MODES_GENERIC)}")
            if mode not in _lib.REGRESS_MODES_GENERIC:
                raise ValueError(f"unknown regressor mode {mode!r}: one of {sorted(_lib.REGRESS_MODES_GENERIC)} for a generic regressor")
            with torch.cuda.device(self.device):
                _lib.check(_lib.p2p_regressor_set_mode(self.handle, _lib.REGRESS_MODES_GENERIC[mode]), "p2p_regressor_set_mode")
            return
        if mode in _lib.REGRESS_MODES_GENERIC:
            raise NotImplementedError(f"regressor mode {mode!r} needs a generic regressor (a non-released configuration, or generic=True)")
        if mode not in modes:
            removed = {"bf16x2": "round 5", "bf16x3": "round 4"}
            why = f" ({mode!r} was removed in {removed[mode]})" if mode in removed else ""
            raise ValueError(f"unknown regressor mode {mode!r}{why}: one of {sorted(modes)}")
        # packing another mode's weight stream allocates and copies on the CURRENT device: make that the handle's device
        with torch.cuda.device(self.device):
            _lib.check(_lib.p2p_regressor_set_mode(self.handle, modes[mode]), "p2p_regressor_set_mode")

    @property
    def mode(self):
        code = _lib.p2p_regressor_get_mode(self.handle)
        names = {v: k for k, v in {**_lib.REGRESS_MODES, **_lib.REGRESS_MODES_LOSSY, **_lib.REGRESS_MODES_GENERIC}.items()}
        return names[code]

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.p2p_regressor_destroy(self.handle)
            self.handle = None


_workspaces = {}

# Optional launch timing (bench.py): when a list is installed here, regress() brackets its launch
# with HIP events recorded on the stream the kernel is launched on and appends (start, end, n).
regress_events = None


def _workspace(device, nbytes):
    """One growing scratch buffer per (device, stream)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


# Upper bound on the coarse-stage scratch of one call: a batch whose pairs need more is processed in groups
# (the hidden volume of the consensus net is 184 MB per 480x640 pair, 2.9 GB per 960x1280 pair).
COARSE_WORKSPACE_LIMIT = 16 << 30


def coarse_forward_batch(feat_a, feat_b, ksize, ncn, want_delta=True, out_corr=None, out_delta=None):
    """forward_coarse_match for the B pairs of feat_a [B,C,hA,wA] / feat_b [B,C,hB,wB] (fp32 GPU) in one launch
    per kernel.  Returns (corr [B,hA',wA',hB',wB'], packed delta uint8 of the same shape or None); `out_*` let
    the caller provide (contiguous) outputs."""
    feat_a, feat_b = _f32c(feat_a, "feat_a"), _f32c(feat_b, "feat_b")
    if feat_a.dim() != 4 or feat_b.dim() != 4 or feat_a.shape[0] != feat_b.shape[0]:
        raise ValueError("coarse_forward_batch expects [B,C,h,w] feature maps with equal B")
    nb, c, ha, wa = feat_a.shape
    _, c2, hb, wb = feat_b.shape
    if c != c2:
        raise ValueError("channel mismatch between the two feature maps")
    dev = feat_a.device
    k = max(ksize, 1)
    shape = (nb, ha // k, wa // k, hb // k, wb // k)
    corr = out_corr if out_corr is not None else torch.empty(shape, dtype=torch.float32, device=dev)
    delta = None
    if ksize > 1 and want_delta:
        delta = out_delta if out_delta is not None else torch.empty(shape, dtype=torch.uint8, device=dev)
    assert corr.is_contiguous() and corr.numel() == math.prod(shape) and corr.dtype == torch.float32
    assert delta is None or (delta.is_contiguous() and delta.numel() == math.prod(shape) and delta.dtype == torch.uint8)
    if nb == 0:
        return corr, delta
    with torch.cuda.device(dev):
        per_pair = _lib.p2p_coarse_workspace_bytes_for(ncn.handle, c, ha, wa, hb, wb, ksize)
        if per_pair == 0:
            raise ValueError("coarse_forward: bad sizes")
        pairs = max(1, min(nb, COARSE_WORKSPACE_LIMIT // per_pair))
        ws = _workspace(dev, pairs * per_pair)
        _lib.check(_lib.p2p_coarse_forward_batch(feat_a.data_ptr(), feat_b.data_ptr(), nb, c, ha, wa, hb, wb, ksize,
                                                 ncn.handle, corr.data_ptr(),
                                                 delta.data_ptr() if delta is not None else None,
                                                 ws.data_ptr(), ws.numel(), _stream()), "p2p_coarse_forward_batch")
    return corr, delta


def coarse_forward(feat_a, feat_b, ksize, ncn, want_delta=True, out_corr=None, out_delta=None):
    """forward_coarse_match for one pair.  feat_*: [C,h,w] fp32 GPU.  Returns (corr [hA',wA',hB',wB'],
    packed delta uint8 of the same shape or None)."""
    corr, delta = coarse_forward_batch(feat_a[None], feat_b[None], ksize, ncn, want_delta,
                                       out_corr[None] if out_corr is not None else None,
                                       out_delta[None] if out_delta is not None else None)
    return corr[0], (delta[0] if delta is not None else None)


def neigh_consensus_batch(x, ncn):
    """NeighConsensus.forward (reference networks/ncn/model.py:145-155) on a batch of volumes x [B,hA,wA,hB,wB] fp32 GPU
    -> the same shape: both consensus layers and both symmetric branches in one kernel (csrc/consensus.hip), or a generic
    handle's stack layer by layer (csrc/consensus_generic.hip)."""
    x = _f32c(x, "x")
    if x.dim() != 5:
        raise ValueError("neigh_consensus_batch expects [B,hA,wA,hB,wB]")
    nb, ha, wa, hb, wb = x.shape
    y = torch.empty_like(x)
    if nb == 0 or x.numel() == 0:
        return y
    with torch.cuda.device(x.device):
        per = _lib.p2p_neigh_consensus_workspace_bytes(ncn.handle, ha, wa, hb, wb)
        nbytes = per * max(1, min(nb, COARSE_WORKSPACE_LIMIT // per))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.p2p_neigh_consensus_batch(x.data_ptr(), nb, ha, wa, hb, wb, ncn.handle, y.data_ptr(), ws.data_ptr(), nbytes,
                                                  _stream()), "p2p_neigh_consensus_batch")
    return y


def delta_unpack(delta, ksize):
    """Packed argmax byte -> the reference's (max_i, max_j, max_k, max_l) int64 tensors."""
    out = torch.empty((4,) + tuple(delta.shape), dtype=torch.int64, device=delta.device)
    if delta.numel() == 0:
        return out[0], out[1], out[2], out[3]
    with torch.cuda.device(delta.device):
        _lib.check(_lib.p2p_delta_unpack(delta.data_ptr(), delta.numel(), ksize, out.data_ptr(), _stream()),
                   "p2p_delta_unpack")
    return out[0], out[1], out[2], out[3]


def coarse_matches_batch(corr, delta, ksize, upsample, center=True, out_matches=None, out_scores=None):
    """cal_coarse_matches for B pairs: corr [B,hA',wA',hB',wB'] (+ packed delta of the same shape or None) ->
    ([B,nB+nA,4] int64 pixel matches, [B,nB+nA] fp32 scores)."""
    corr = _f32c(corr, "corr4d")
    if corr.dim() != 5:
        raise ValueError("coarse_matches_batch expects corr4d of shape [B,hA,wA,hB,wB]")
    nb, ha, wa, hb, wb = corr.shape
    n = ha * wa + hb * wb
    dev = corr.device
    matches = out_matches if out_matches is not None else torch.empty((nb, n, 4), dtype=torch.int64, device=dev)
    scores = out_scores if out_scores is not None else torch.empty((nb, n), dtype=torch.float32, device=dev)
    assert matches.is_contiguous() and matches.numel() == nb * n * 4 and matches.dtype == torch.int64
    assert scores.is_contiguous() and scores.numel() == nb * n and scores.dtype == torch.float32
    if delta is not None:
        delta = delta.contiguous()
        if delta.dtype != torch.uint8 or delta.numel() != corr.numel():
            raise ValueError("delta must be the packed uint8 volume with the shape of corr4d")
    if nb == 0:
        return matches, scores
    with torch.cuda.device(dev):
        _lib.check(_lib.p2p_coarse_matches_batch(corr.data_ptr(), delta.data_ptr() if delta is not None else None, nb,
                                                 ha, wa, hb, wb, ksize, upsample, int(bool(center)),
                                                 matches.data_ptr(), scores.data_ptr(), _stream()),
                   "p2p_coarse_matches_batch")
    return matches, scores


def coarse_matches(corr, delta, ksize, upsample, center=True, out_matches=None, out_scores=None):
    """cal_coarse_matches for one pair: ([nB+nA,4] int64 pixel matches, [nB+nA] fp32 scores)."""
    m, sc = coarse_matches_batch(corr[None], delta[None] if delta is not None else None, ksize, upsample, center,
                                 out_matches[None] if out_matches is not None else None,
                                 out_scores[None] if out_scores is not None else None)
    return m[0], sc[0]


def coarse_matches_topk_batch(corr, delta, ksize, upsample, center, topk, do_softmax=True):
    """The topk best candidates per cell and direction (corr_to_matches_topk in both directions, concatenated like
    cal_coarse_matches): corr [B,hA',wA',hB',wB'] (+ packed delta or None) -> ([B,topk*(nB+nA),4] int64 pixel matches,
    [B,topk*(nB+nA)] fp32 scores).  Row order and tie rule: include/p2p_hip.h.  do_softmax=False: raw consensus values."""
    corr = _f32c(corr, "corr4d")
    if corr.dim() != 5:
        raise ValueError("coarse_matches_topk_batch expects corr4d of shape [B,hA,wA,hB,wB]")
    nb, ha, wa, hb, wb = corr.shape
    topk = int(topk)
    n = max(topk, 0) * (ha * wa + hb * wb)
    dev = corr.device
    matches = torch.empty((nb, n, 4), dtype=torch.int64, device=dev)
    scores = torch.empty((nb, n), dtype=torch.float32, device=dev)
    if delta is not None:
        delta = delta.contiguous()
        if delta.dtype != torch.uint8 or delta.numel() != corr.numel():
            raise ValueError("delta must be the packed uint8 volume with the shape of corr4d")
    if nb == 0:
        return matches, scores
    with torch.cuda.device(dev):
        _lib.check(_lib.p2p_coarse_matches_topk_batch(corr.data_ptr(), delta.data_ptr() if delta is not None else None, nb,
                                                      ha, wa, hb, wb, ksize, upsample, int(bool(center)), topk,
                                                      int(bool(do_softmax)), matches.data_ptr(), scores.data_ptr(), _stream()),
                   "p2p_coarse_matches_topk_batch")
    return matches, scores


def score_norm(normalize):
    """`normalize` of cal_coarse_score (None, 'softmax' or 'l1') -> P2P_SCORE_*; anything else raises ValueError (the
    reference goes on to call the string and fails with a TypeError).  No GPU needed."""
    if normalize is not None and not isinstance(normalize, str) or normalize not in _lib.SCORE_NORMS:
        raise ValueError(f"normalize must be None, 'softmax' or 'l1', got {normalize!r}")
    return _lib.SCORE_NORMS[normalize]


def coarse_score_batch(corr, normalize="softmax", return_cells=False):
    """cal_coarse_score (reference networks/patch2pix.py:320-338) per pair: corr [B,hA',wA',hB',wB'] fp32 GPU -> [B] fp32, the
    mean over the nA + nB cells of both images of the best normalised consensus value (normalize: None, 'softmax', 'l1').
    return_cells: also the cell scores [B, nA+nB], A cells first (the reference's torch.cat([scores_A, scores_B])).  A
    pair's scores do not depend on the batch (include/p2p_hip.h)."""
    norm = score_norm(normalize)
    corr = _f32c(corr, "corr4d")
    if corr.dim() != 5:
        raise ValueError("coarse_score_batch expects corr4d of shape [B,hA,wA,hB,wB]")
    nb, ha, wa, hb, wb = corr.shape
    dev = corr.device
    pair = torch.empty((nb,), dtype=torch.float32, device=dev)
    cells = torch.empty((nb, ha * wa + hb * wb), dtype=torch.float32, device=dev)      # stream-ordered scratch when not returned
    if nb:
        with torch.cuda.device(dev):
            _lib.check(_lib.p2p_coarse_score_batch(corr.data_ptr(), nb, ha, wa, hb, wb, norm, cells.data_ptr(), pair.data_ptr(),
                                                   None, 0, _stream()), "p2p_coarse_score_batch")
    return (pair, cells) if return_cells else pair


def filter_coarse_batch(matches, scores, ncn_thres=0.0, mutual=True):
    """filter_coarse (networks/utils.py:38-72, no ptmax) on the device for a batch: matches [B,n,4] int64, scores [B,n]
    fp32 -> (rows [B,n,4], scores [B,n], counts int32 [B]); the first counts[b] rows of item b are valid, in the
    reference's order.  counts[b] == -1 asks for the host path (a coordinate outside [0, 2^15)).  Any n up to 2^20:
    lists longer than 8192 rows are sorted through a scratch buffer (16 bytes per padded row)."""
    if matches.dtype != torch.int64 or matches.dim() != 3 or matches.shape[-1] != 4 or not matches.is_cuda:
        raise TypeError("matches must be an int64 [B,n,4] tensor on the GPU")
    scores = _f32c(scores, "scores")
    matches = matches.contiguous()
    nb, n, _ = matches.shape
    dev = matches.device
    out_m, out_s = torch.empty_like(matches), torch.empty_like(scores)
    counts = torch.empty((nb,), dtype=torch.int32, device=dev)
    if nb and n:
        with torch.cuda.device(dev):
            need = _lib.p2p_filter_coarse_workspace_bytes(nb, n)
            ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None      # stream-ordered by the allocator
            _lib.check(_lib.p2p_filter_coarse_batch(matches.data_ptr(), scores.data_ptr(), nb, n, float(ncn_thres),
                                                    int(bool(mutual)), out_m.data_ptr(), out_s.data_ptr(),
                                                    counts.data_ptr(), ws.data_ptr() if need else None, need, _stream()),
                       "p2p_filter_coarse_batch")
    else:
        counts.zero_()
    return out_m, out_s, counts


_small_ring = staging.PinnedRing(8)


def small_to_device(array, dtype, device):
    """A small host array -> device tensor through the pinned staging ring (staging.py), asynchronously.  A copy from
    pageable memory makes the host wait for everything queued on the stream before it; a caller that pipelines batches
    must never do that."""
    return staging.upload([torch.as_tensor(array, dtype=dtype)], device, _small_ring)[0]


def match_tail_batch(fine, scores, coarse, counts, scale, io_thres):
    """The tail of estimate_matches (utils/eval/model_helper.py:92-109) on the device for padded batch outputs:
    fine [B,n,4] fp32, scores [B,n] fp32, coarse [B,n,4] int64, counts int32 [B] (device), scale [B,4] float64 ->
    (matches [B,n,4] float64, scores [B,n] fp32, coarse [B,n,4] float64, counts int32 [B]); rows with score > io_thres
    are kept in order (all rows if none passes) and scaled to original-image pixels."""
    if fine.dtype != torch.float32 or coarse.dtype != torch.int64 or counts.dtype != torch.int32 or not fine.is_cuda:
        raise TypeError("match_tail_batch: fine fp32, coarse int64, counts int32 on the GPU expected")
    fine, scores, coarse = fine.contiguous(), _f32c(scores, "scores"), coarse.contiguous()
    nb, n, _ = fine.shape
    dev = fine.device
    scale = scale.to(torch.float64).reshape(nb, 4) if torch.is_tensor(scale) and scale.is_cuda else \
        small_to_device(torch.as_tensor(scale, dtype=torch.float64).reshape(nb, 4), torch.float64, dev)
    out_m = torch.empty((nb, n, 4), dtype=torch.float64, device=dev)
    out_c = torch.empty((nb, n, 4), dtype=torch.float64, device=dev)
    out_s = torch.empty((nb, n), dtype=torch.float32, device=dev)
    out_n = torch.empty((nb,), dtype=torch.int32, device=dev)
    if nb and n:
        with torch.cuda.device(dev):
            _lib.check(_lib.p2p_match_tail_batch(fine.data_ptr(), scores.data_ptr(), coarse.data_ptr(), counts.data_ptr(),
                                                 scale.data_ptr(), nb, n, float(io_thres), out_m.data_ptr(), out_s.data_ptr(),
                                                 out_c.data_ptr(), out_n.data_ptr(), _stream()), "p2p_match_tail_batch")
    else:
        out_n.zero_()
    return out_m, out_s, out_c, out_n


EPI_BINS_MEASURE = [0, 1e-2, 1, 5, 10, 25, 50, 100, 400, 2500, 1e5]      # default of check_inliers_distr (measure.py:116)
EPI_BINS_EVAL = [0, 1e-2, 1, 5, 10, 25, 50, 100, 2500, 1e5]              # what eval_epoch_immatch.py:85 passes


def epi_kind(kind):
    """`kind` of epipolar_batch ('sampson', 'sym', 'sym_sqrt', or 'value' for distances that are only binned) -> P2P_EPI_*; anything else raises ValueError.  No GPU needed."""
    if not isinstance(kind, str) or kind not in _lib.EPI_KINDS:
        raise ValueError(f"kind must be one of {sorted(_lib.EPI_KINDS)}, got {kind!r}")
    return _lib.EPI_KINDS[kind]


def epi_edges(bins):
    """The nbins + 1 bin edges of epipolar_batch as a float64 array, checked where they still are on the host: one dimension,
    2 to 17 values, no NaN, ascending (np.histogram's own condition).  ValueError otherwise; more than 16 bins
    NotImplementedError.  No GPU needed."""
    edges = np.asarray(bins, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError(f"bins must be a one-dimensional sequence of at least two edges, got shape {edges.shape}")
    if np.isnan(edges).any() or bool((np.diff(edges) < 0).any()):
        raise ValueError("bins must increase monotonically and hold no NaN")
    if edges.size - 1 > _lib.EPI_MAX_BINS:
        raise NotImplementedError(f"{edges.size - 1} bins: at most {_lib.EPI_MAX_BINS} are implemented")
    return edges


def epipolar_batch(matches, counts, F, kind="sampson", eps=1e-8, bins=None, out_dtype=None):
    """Distances of match rows to the epipolar geometry of their pair's fundamental matrix, and their bin counts, on the device
    (reference utils/eval/measure.py:18-71,115-141 and networks/utils.py:74-110; include/p2p_hip.h, p2p_epipolar_batch):
    matches [B,n,4] float64, float32 or int64 on the GPU (x1, y1, x2, y2), counts int32 [B] on the GPU (valid rows per item; -1
    passes through) or None (all n rows), F [B,3,3] or [3,3] (x2^T F x1 = 0; a single matrix serves B = 1), kind 'sampson' |
    'sym' | 'sym_sqrt', eps 0 for the numpy symmetric distance, bins a host sequence of ascending edges or None.
    -> (dist [B,n] of out_dtype (default float64), rows beyond counts[b] zero; hist int32 [B,nbins] or None)."""
    code = epi_kind(kind)
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f"eps must be >= 0, got {eps!r}")
    edges = epi_edges(bins) if bins is not None else None
    if not torch.is_tensor(matches) or matches.dim() != 3 or matches.shape[-1] != 4:
        raise ValueError("matches must be a [B,n,4] tensor")
    nb, n, _ = matches.shape
    F = torch.as_tensor(F)
    if tuple(F.shape) == (3, 3) and nb == 1:
        F = F[None]
    if tuple(F.shape) != (nb, 3, 3):
        raise ValueError(f"F must have shape [{nb},3,3] (or [3,3] for one item), got {tuple(F.shape)}")
    out_dtype = torch.float64 if out_dtype is None else out_dtype
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError(f"out_dtype must be torch.float64 or torch.float32, got {out_dtype}")
    if counts is not None and (not torch.is_tensor(counts) or counts.numel() != nb):
        raise ValueError(f"counts must be an int32 tensor of {nb} values or None")
    name = str(matches.dtype).replace("torch.", "")
    if name not in _lib.DTYPES or not matches.is_cuda:
        raise TypeError(f"matches must be a float64, float32 or int64 tensor on the GPU (got {matches.dtype}, {matches.device})")
    if counts is not None and (counts.dtype != torch.int32 or counts.device != matches.device):
        raise TypeError("counts must be an int32 tensor on the device of matches")
    dev = matches.device
    matches = matches.contiguous()
    dist = torch.zeros((nb, n), dtype=out_dtype, device=dev)
    hist = torch.zeros((nb, len(edges) - 1), dtype=torch.int32, device=dev) if edges is not None else None
    if nb == 0 or n == 0:
        return dist, hist
    if nb > 65535:
        raise ValueError(f"epipolar_batch: {nb} items (at most 65535 per call)")
    with torch.cuda.device(dev):
        if F.is_cuda:
            Fd = F.to(dev, torch.float64).contiguous()
            dedges = small_to_device(edges, torch.float64, dev) if edges is not None else None
        else:          # F and the edges in ONE copy through the staging ring
            parts = [F.to(torch.float64).contiguous()] + ([torch.from_numpy(edges)] if edges is not None else [])
            up = staging.upload(parts, dev, _small_ring)
            Fd, dedges = up[0], (up[1] if edges is not None else None)
        if counts is None:
            counts = torch.full((nb,), n, dtype=torch.int32, device=dev)
        counts = counts.contiguous()
        _lib.check(_lib.p2p_epipolar_batch(matches.data_ptr(), _lib.DTYPES[name], counts.data_ptr(), Fd.data_ptr(), nb, n,
                                           code, eps, dedges.data_ptr() if edges is not None else None,
                                           len(edges) - 1 if edges is not None else 0, dist.data_ptr(),
                                           _lib.DTYPES[str(out_dtype).replace("torch.", "")],
                                           hist.data_ptr() if hist is not None else None, _stream()), "p2p_epipolar_batch")
    return dist, hist


def regress_batch_dev(reg1, reg2, pyrs1, pyrs2, proposals, counts, want_raw=False, out=None):
    """regress_batch with the proposal counts in device memory: proposals [B,stride,4] (int64 or float32), counts int32
    [B] on the GPU; every output is padded to [B,stride,...], rows beyond counts[b] are left uninitialised -- or, with
    `out` (a dict of contiguous float32 buffers of those shapes by output name), as the caller filled them."""
    nb, stride, _ = proposals.shape
    dev = proposals.device
    if proposals.dtype not in (torch.int64, torch.float32):
        raise TypeError("proposals must be int64 or float32")
    if counts.dtype != torch.int32 or counts.numel() != nb or not counts.is_cuda:
        raise TypeError("counts must be an int32 [B] tensor on the GPU")
    proposals = proposals.contiguous()
    pyr_a, pyr_b, keep = (_lib.Pyramid * nb)(), (_lib.Pyramid * nb)(), []
    for i in range(nb):
        pa, ka = _pyramid(pyrs1[i], reg1.layout["feat_idx"])
        pb, kb = _pyramid(pyrs2[i], reg1.layout["feat_idx"])
        pyr_a[i], pyr_b[i] = pa, pb
        keep.append((ka, kb))
    given = out or {}
    two = reg2 is not None
    out = {"matches1": torch.empty((nb, stride, 4), device=dev), "probs1": torch.empty((nb, stride), device=dev)}
    if two:
        out["matches2"], out["probs2"] = torch.empty((nb, stride, 4), device=dev), torch.empty((nb, stride), device=dev)
    if want_raw:
        out["raw1"] = torch.empty((nb, stride, 5), device=dev)
        if two:
            out["raw2"] = torch.empty((nb, stride, 5), device=dev)
    for k in out:
        if k in given:
            if given[k].shape != out[k].shape or given[k].dtype != torch.float32 or not given[k].is_contiguous() or given[k].device != dev:
                raise ValueError(f"out[{k!r}] must be a contiguous float32 tensor of shape {tuple(out[k].shape)} on {dev}")
            out[k] = given[k]
    g = lambda k: out[k].data_ptr() if k in out else None
    if nb and stride:
        with torch.cuda.device(dev):
            ws = _regress_scratch(dev, nb * stride, reg1)
            _lib.check(_lib.p2p_regress_batch_dev(reg1.handle, reg2.handle if two else None, nb, pyr_a, pyr_b,
                                                  counts.data_ptr(), stride, proposals.data_ptr(),
                                                  int(proposals.is_floating_point()), g("matches1"), g("probs1"), g("raw1"),
                                                  g("matches2"), g("probs2"), g("raw2"), ws.data_ptr(), ws.numel(), _stream()),
                       "p2p_regress_batch_dev")
    del keep
    return out


# Tests and tools: a cap (bytes) on the scratch handed to a GENERIC regressor, which cuts its chunks to what it is given
# (at least p2p_regress_workspace_bytes_for(handle, 8); results do not depend on it).
generic_scratch_limit = None


def _regress_scratch(dev, n, reg=None):
    """Scratch of one regress call (the pooled convolution features wait there for the batched FC tail; in the default mode
    also the Winograd-transformed input of the second convolution, chunk by chunk): a fresh stream-ordered allocation per
    call, so that calls on different streams never share it; sized for the regressor's arithmetic mode."""
    if reg is None:
        nbytes = _lib.p2p_regress_workspace_bytes(int(n))
    else:
        nbytes = _lib.p2p_regress_workspace_bytes_for(reg.handle, int(n))
        if generic_scratch_limit is not None and getattr(reg, "generic", False):
            nbytes = min(nbytes, int(generic_scratch_limit))
    return torch.empty(max(int(nbytes), 128), dtype=torch.uint8, device=dev)


def _pyramid(levels, used=(0, 1, 2, 3)):
    """used: the levels the regressor reads (its feat_idx).  Only those are held to the 3 / 64 / 64 / 128 channels the library
    gathers; a level it never reads (levels 2, 3 of a Bottleneck pyramid under feat_idx within {0, 1}) travels as a pointer."""
    if len(levels) != 4:
        raise ValueError("a pyramid is the 4 maps of feat_idx [0,1,2,3]")
    lv = [_f32c(t, "pyramid level") for t in levels]
    h, w = lv[0].shape[-2:]
    if h < 8 or w < 8:
        raise ValueError(f"images must be at least 8x8 pixels (got {h}x{w})")
    up = lambda d, j: (d + (1 << j) - 1) >> j          # the backbone's strided layers round up (resnet.py)
    exp = [(3, h, w), (64, up(h, 1), up(w, 1)), (64, up(h, 2), up(w, 2)), (128, up(h, 3), up(w, 3))]
    for j, (t, e) in enumerate(zip(lv, exp)):
        if j in used and tuple(t.shape) != e:
            raise ValueError(f"pyramid level has shape {tuple(t.shape)}, expected {e}")
    p = _lib.Pyramid()
    for j in range(4):
        p.level[j] = lv[j].data_ptr()
    p.height, p.width = h, w
    return p, lv


def regress_batch(reg1, reg2, pyrs1, pyrs2, proposals, want_mid=True, want_raw=False):
    """forward_fine_match for a list of pairs in ONE launch; with reg2 the mid->fine chain runs inside it.

    pyrs1/pyrs2: per pair, the 4 maps of feat_idx [0,1,2,3]; proposals: per pair [n_i,4] int64 or
    float32 (same dtype for all).  Returns a list of dicts 'matches1','probs1' (+ 'matches2','probs2'
    when reg2 is given; 'raw*' on request), views into shared buffers."""
    nitems = len(proposals)
    if nitems == 0:
        return []
    dev = proposals[0].device
    dtype = proposals[0].dtype
    if dtype == torch.int64:
        is_float = 0
    elif dtype == torch.float32:
        is_float = 1
    else:
        raise TypeError("proposals must be int64 or float32")
    if any(p.dtype != dtype for p in proposals):
        raise TypeError("all proposal arrays of a batch must share one dtype")
    counts = [int(p.shape[0]) for p in proposals]
    n = sum(counts)
    allp = proposals[0].contiguous() if nitems == 1 else torch.cat([p.reshape(-1, 4) for p in proposals])
    pyr_a = (_lib.Pyramid * nitems)()
    pyr_b = (_lib.Pyramid * nitems)()
    keep = []
    for i in range(nitems):
        pa, ka = _pyramid(pyrs1[i], reg1.layout["feat_idx"])
        pb, kb = _pyramid(pyrs2[i], reg1.layout["feat_idx"])
        pyr_a[i], pyr_b[i] = pa, pb
        keep.append((ka, kb))
    cnt = (ctypes.c_int * nitems)(*counts)
    bufs = {}

    def buf(key, cols, cond=True):
        if not cond:
            return None
        bufs[key] = torch.empty((n, cols) if cols > 1 else (n,), dtype=torch.float32, device=dev)
        return bufs[key].data_ptr()

    two = reg2 is not None
    m1 = buf("matches1", 4, want_mid or not two)
    q1 = buf("probs1", 1, want_mid or not two)
    r1 = buf("raw1", 5, want_raw)
    m2 = buf("matches2", 4, two)
    q2 = buf("probs2", 1, two)
    r2 = buf("raw2", 5, two and want_raw)
    if n:
        with torch.cuda.device(dev):
            ws = _regress_scratch(dev, n, reg1)
            ev = None
            if regress_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            _lib.check(_lib.p2p_regress_batch(reg1.handle, reg2.handle if two else None, nitems, pyr_a, pyr_b, cnt,
                                              allp.data_ptr(), is_float, m1, q1, r1, m2, q2, r2, ws.data_ptr(), ws.numel(),
                                              _stream()), "p2p_regress_batch")
            if ev is not None:
                ev[1].record()
                regress_events.append((ev[0], ev[1], n, 2 if two else 1))
    del keep
    outs, start = [], 0
    for c in counts:
        outs.append({k: v[start:start + c] for k, v in bufs.items()})
        start += c
    return outs


def regress(reg1, reg2, pyr1, pyr2, proposals, want_mid=True, want_raw=False):
    """Single-pair form of regress_batch (returns one dict)."""
    return regress_batch(reg1, reg2, [pyr1], [pyr2], [proposals], want_mid, want_raw)[0]


# ---- the matching operators on their own (networks.modules, networks.ncn.*) -------------------------------------------------
def _op_input(t, name, dim=None):
    """Inference only, on the GPU: what every operator front end asks of an input tensor."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on the GPU (got {t.device}): the operators have no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} requires grad: the operators are inference only (wrap the call in torch.no_grad())")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"{name} must have {dim} dimensions (got {tuple(t.shape)})")
    return t.detach().contiguous()


def correlation_batch(feat_a, feat_b):
    """FeatCorrelation (modules.py:41-53): feat_a [B,C,hA,wA], feat_b [B,C,hB,wB] -> [B, hA*wA, hB*wB], exact fp32 MFMA."""
    feat_a, feat_b = _op_input(feat_a, "feat1", 4), _op_input(feat_b, "feat2", 4)
    if feat_a.shape[:2] != feat_b.shape[:2] or feat_a.device != feat_b.device:
        raise ValueError(f"feature maps {tuple(feat_a.shape)} and {tuple(feat_b.shape)} must agree in batch, channels and device")
    nb, c, ha, wa = feat_a.shape
    hb, wb = feat_b.shape[2:]
    out = torch.empty((nb, ha * wa, hb * wb), dtype=torch.float32, device=feat_a.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(feat_a.device):
        _lib.check(_lib.p2p_correlation_batch(feat_a.data_ptr(), feat_b.data_ptr(), nb, c, ha, wa, hb, wb, out.data_ptr(), _stream()),
                   "p2p_correlation_batch")
    return out


def maxpool4d_batch(x, k, want_delta=True):
    """maxpool4d (modules.py:11-34) of x [B,H1,W1,H2,W2] -> (pooled [B,H1/k,...], packed delta uint8 of that shape or None)."""
    x = _op_input(x, "corr4d_hres", 5)
    nb, h1, w1, h2, w2 = x.shape
    k = int(k)
    shape = (nb, h1 // k, w1 // k, h2 // k, w2 // k) if k > 0 else (nb, 0, 0, 0, 0)
    pooled = torch.empty(shape, dtype=torch.float32, device=x.device)
    delta = torch.empty(shape, dtype=torch.uint8, device=x.device) if want_delta else None
    if x.numel() == 0 and k > 0:
        return pooled, delta
    with torch.cuda.device(x.device):
        _lib.check(_lib.p2p_maxpool4d_batch(x.data_ptr(), nb, h1, w1, h2, w2, k, pooled.data_ptr(),
                                            delta.data_ptr() if want_delta else None, _stream()), "p2p_maxpool4d_batch")
    return pooled, delta


def mutual_matching_batch(x):
    """MutualMatching (ncn/model.py:157-176) of x [B,hA,wA,hB,wB] -> the same shape."""
    x = _op_input(x, "corr4d", 5)
    nb, ha, wa, hb, wb = x.shape
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    with torch.cuda.device(x.device):
        nbytes = _lib.p2p_mutual_matching_workspace_bytes(nb, ha, wa, hb, wb)
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=x.device)
        _lib.check(_lib.p2p_mutual_matching_batch(x.data_ptr(), nb, ha, wa, hb, wb, y.data_ptr(), ws.data_ptr(), nbytes, _stream()),
                   "p2p_mutual_matching_batch")
    return y


def l2_normalize(x, dim):
    """L2Normalize (modules.py:6) of x along `dim`."""
    x = _op_input(x, "feat")
    dim = dim % x.dim()
    outer, c, inner = math.prod(x.shape[:dim]), x.shape[dim], math.prod(x.shape[dim + 1:])
    y = torch.empty_like(x)
    if x.numel() == 0:
        return y
    with torch.cuda.device(x.device):
        _lib.check(_lib.p2p_l2_normalize(x.data_ptr(), outer, c, inner, y.data_ptr(), _stream()), "p2p_l2_normalize")
    return y


class Conv4dWeights:
    """Device-resident filters of one Conv4d layer (conv4d.py:77-130): weight in the stored layout [k, c_out, c_in, k, k, k]."""

    def __init__(self, weight, bias, device):
        w = _host(weight)
        if w.dim() != 6 or len({w.shape[0], w.shape[3], w.shape[4], w.shape[5]}) != 1:
            raise ValueError(f"Conv4d weight has shape {tuple(w.shape)}: expected the stored layout [k, c_out, c_in, k, k, k]")
        b = _host(bias) if bias is not None else None
        if b is not None and tuple(b.shape) != (w.shape[1],):
            raise ValueError(f"Conv4d bias has shape {tuple(b.shape)}: expected ({w.shape[1]},)")
        self.c_in, self.c_out, self.k = int(w.shape[2]), int(w.shape[1]), int(w.shape[0])
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.p2p_conv4d_create(w.data_ptr(), b.data_ptr() if b is not None else None, self.c_in, self.c_out, self.k,
                                              ctypes.byref(self.handle)), "p2p_conv4d_create")
        self.device = torch.device(device)

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.p2p_conv4d_destroy(self.handle)
            self.handle = None


def conv4d_forward_batch(x, conv):
    """One Conv4d layer: x [B,c_in,h1,w1,h2,w2] -> [B,c_out,h1,w1,h2,w2] (bias, no ReLU), exact fp32 MFMA."""
    x = _op_input(x, "data", 6)
    nb, c, h1, w1, h2, w2 = x.shape
    if c != conv.c_in:
        raise ValueError(f"data has {c} channels, the layer takes {conv.c_in}")
    y = torch.empty((nb, conv.c_out, h1, w1, h2, w2), dtype=torch.float32, device=x.device)
    if y.numel() == 0:
        return y
    with torch.cuda.device(x.device):
        _lib.check(_lib.p2p_conv4d_forward_batch(conv.handle, x.data_ptr(), nb, h1, w1, h2, w2, y.data_ptr(), _stream()),
                   "p2p_conv4d_forward_batch")
    return y


def tensor_signature(tensors):
    """Identity, version counter and storage of every tensor: the key of a packed-weights cache (ResNet34._hip_signature)."""
    return tuple((id(t), t._version, t.data_ptr(), tuple(t.shape), str(t.device)) for t in tensors)
