"""`Patch2Pix` with the reference's public surface (networks/patch2pix.py) on top of libp2p_hip.

Same constructor config, attributes (`device`, `upsample`, `psize`, `panc`, ...), method names,
argument meaning and return layouts as the reference class, so callers such as
utils/eval/model_helper.py (and image-matching-toolbox through it) work unchanged.  The ResNet
backbone (networks/resnet.py) keeps its torch parameters and runs its convolutions through the same
library; everything after the feature pyramid is HIP as well.  Inference only:
`config.training=True` raises (training is out of scope).
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import resnet
from .utils import filter_coarse
from .. import ops, staging


BACKBONES = ("ResNet34", "ResNet50", "ResNet101")      # what `config.backbone` may name (reference networks/resnet.py:175-191)
REGRESSOR_FEAT_DIMS = (3, 64, 64, 128, 256)            # what the reference builds its regressors for, whatever the backbone (patch2pix.py:20)


def backbone_layout(backbone, change_stride, feat_idx=None):
    """What `Patch2Pix(config)` derives from the backbone's name and stride, checked without a GPU:
    -> (class of networks/resnet.py, upsample, feats_downsample).  An unknown name raises NotImplementedError.  `feat_idx` (the
    levels a regressor reads; None: no regressor) must name levels whose channel count is the reference's hard-coded one:
    every level for ResNet34, levels 0 and 1 for the Bottleneck backbones -- ValueError otherwise, naming the level (the
    reference fails there too, later, with a channel mismatch in its first regressor convolution)."""
    if backbone not in BACKBONES:
        raise NotImplementedError(f"backbone {backbone}: one of {', '.join(BACKBONES)} (reference networks/resnet.py:175-191)")
    cls = getattr(resnet, backbone)
    dims = [3, 64] + [planes * cls.block.expansion for _, planes, _, _ in cls.stages]
    for lvl in (feat_idx or ()):
        if 0 <= lvl < len(dims) and dims[lvl] != REGRESSOR_FEAT_DIMS[lvl]:
            raise ValueError(f"feat_idx {list(feat_idx)}: level {lvl} of a {backbone} pyramid has {dims[lvl]} channels, the regressors "
                             f"are built for {REGRESSOR_FEAT_DIMS[lvl]} (reference networks/patch2pix.py:20); use levels within "
                             f"{{0, 1}} with this backbone")
    # stride 8: layer3 keeps the resolution of layer2 (change_stride); else stride 16 -- levels 0..3 are the same either way
    return cls, (8 if change_stride else 16), [1, 2, 2, 2, 1 if change_stride else 2]


class _Holder(nn.Module):
    """Parameter container that reproduces a sub-tree of the reference state_dict."""

    def __init__(self, spec):
        super().__init__()
        children = {}
        for name, (shape, kind) in spec.items():
            head, _, rest = name.partition(".")
            if rest:
                children.setdefault(head, {})[rest] = (shape, kind)
            elif kind == "param":
                self.register_parameter(head, nn.Parameter(torch.zeros(shape), requires_grad=False))
            else:
                dtype = torch.int64 if kind == "long" else torch.float32
                self.register_buffer(head, torch.zeros(shape, dtype=dtype))
        for head, sub in children.items():
            self.add_module(head, _Holder(sub))


def _bn_spec(prefix, n):
    return {f"{prefix}.weight": ((n,), "param"), f"{prefix}.bias": ((n,), "param"),
            f"{prefix}.running_mean": ((n,), "buffer"), f"{prefix}.running_var": ((n,), "buffer"),
            f"{prefix}.num_batches_tracked": ((), "long")}


def _regressor_spec(layout):
    """Keys and shapes of the reference's FeatRegressNet (networks/modules.py:76-99) for a checked configuration
    (ops.regressor_layout)."""
    shapes, bns = ops.regressor_shapes(layout)
    spec = {k: (shp, "param") for k, shp in shapes.items()}
    for prefix, n in bns.items():
        spec.update(_bn_spec(prefix, n))
    return spec


def _ncn_spec(layout):
    """Keys and shapes of the reference's NeighConsensus (networks/ncn/model.py:124-143, filters in the stored layout of
    conv4d.py:119-120) for a checked stack (ops.ncn_layout)."""
    return {k: (shp, "param") for k, shp in ops.ncn_shapes(layout).items()}


def _ncn_layout_of(config):
    """`config.ncn_config` (namespace or dict: kernel_sizes, channels, optionally symmetric_mode) if present; else the stack
    the checkpoint's ncn.conv.* tensors have; else the released one."""
    nc = getattr(config, "ncn_config", None)
    if nc is not None:
        return ops.ncn_layout(nc)
    wd = getattr(config, "weights_dict", None) or {}
    sub = {k[len("ncn."):]: v for k, v in wd.items() if k.startswith("ncn.conv.")}
    return ops.ncn_layout(sub if sub else None)


_NCN_SPEC = _ncn_spec(ops.RELEASED_NCN_LAYOUT)


class Delta4d:
    """The reference's `delta4d` tuple (max_i, max_j, max_k, max_l), each int64 [B,1,h1,w1,h2,w2]
    (networks/modules.py:24-34), kept packed (one byte per cell) until somebody indexes it."""

    def __init__(self, packed, ksize):
        self.packed = packed            # uint8 [B,h1,w1,h2,w2]
        self.ksize = ksize
        self._planes = None

    def _materialise(self):
        if self._planes is None:
            planes = ops.delta_unpack(self.packed, self.ksize)          # four int64 [B,h1,w1,h2,w2]
            self._planes = tuple(p.unsqueeze(1) for p in planes)
        return self._planes

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return self._materialise()[i]


class Patch2Pix(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.device = torch.device(config.device)
        if self.device.type != "cuda":
            raise RuntimeError("patch2pix_amd runs the matching path on an MI355X; no CPU fallback exists "
                               f"(config.device={config.device})")
        if getattr(config, "training", False):
            raise NotImplementedError("training is out of scope of the MI355X matching path")
        self.backbone = config.backbone
        self.change_stride = config.change_stride
        cls, self.upsample, self.feats_downsample = backbone_layout(
            self.backbone, self.change_stride, config.feat_idx if config.regressor_config else None)
        feat_dims = list(REGRESSOR_FEAT_DIMS)
        self.extract = cls()
        if self.change_stride:
            self.extract.change_stride(target="layer3")
        # what the library implements (include/p2p_hip.h, p2p_ncn_config): NotImplementedError / ValueError otherwise
        self._ncn_layout = _ncn_layout_of(config)
        self.ncn = _Holder(_ncn_spec(self._ncn_layout))

        self.regressor_config = config.regressor_config
        self.regress_mid = None
        self.regress_fine = None
        if self.regressor_config:
            rc = self.regressor_config
            self.regr_batch = config.regr_batch
            self.feat_idx = list(config.feat_idx)
            # what the library implements (include/p2p_hip.h, p2p_regressor_config): NotImplementedError / ValueError otherwise
            self._layout = ops.regressor_layout(rc, self.feat_idx)
            rc.feat_dim = sum(feat_dims[i] for i in self.feat_idx)
            self.ptype = ["center", "center"]
            self.psize = rc.psize
            self.pshift = rc.pshift
            self.panc = rc.panc
            self.shared = rc.shared
            self.regress_mid = _Holder(_regressor_spec(self._layout))
            self.regress_fine = self.regress_mid if self.shared else _Holder(_regressor_spec(self._layout))
        self.to(self.device)
        self._packed = None
        self._ticket_ring = staging.PinnedRing(4)        # up to 4 tickets in flight
        self.init_weights_(weights_dict=config.weights_dict)
        self.eval()

    # ------------------------------------------------------------------ weights
    def init_weights_(self, weights_dict=None, pretrained=True):
        """Load a reference state_dict (networks/patch2pix.py:98-109).  `extract.layer4.*` and any other
        key this inference-only model does not own is ignored, like the reference's strict=False branch."""
        if weights_dict:
            own = self.state_dict()
            picked = {k: v for k, v in weights_dict.items() if k in own}
            missing = [k for k in own if k not in picked and not k.endswith("num_batches_tracked")]
            if missing and any(not k.startswith("extract.") for k in missing) and any(
                    k.startswith(("ncn.", "regress_")) for k in weights_dict):
                raise KeyError(f"checkpoint lacks hot-path weights: {missing[:5]} ...")
            self.load_state_dict(picked, strict=False)
            if not any(k.startswith(("ncn.", "regress_")) for k in picked):
                import warnings
                warnings.warn("Patch2Pix: the checkpoint holds none of the ncn.* / regress_* weights; the matching path keeps "
                              "its initial (zero) parameters and its matches are meaningless", RuntimeWarning)
        self._packed = None

    def load_state_dict(self, *args, **kwargs):
        self._packed = None
        return super().load_state_dict(*args, **kwargs)

    def _weights(self):
        """Pack (BN folding, MFMA fragment order, transposed-branch filters) once per weight load."""
        if self._packed is None:
            sd = self.state_dict()
            ncn = ops.NcnWeights.from_state_dict({k[len("ncn."):]: v for k, v in sd.items() if k.startswith("ncn.")}, self.device,
                                                 symmetric_mode=self._ncn_layout["symmetric_mode"])
            if getattr(self, "_coarse_mode", None) is not None:       # the new handle starts in the default mode
                ncn.set_mode(self._coarse_mode)
            mid = fine = None
            if self.regress_mid is not None:
                sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
                mid = ops.RegressorWeights(sub("regress_mid."), self.device, self.regressor_config, self.feat_idx)
                fine = mid if self.shared else ops.RegressorWeights(sub("regress_fine."), self.device,
                                                                    self.regressor_config, self.feat_idx)
                if getattr(self, "_fine_mode", None) is not None:     # the new handles start in their default mode
                    for reg in {id(mid): mid, id(fine): fine}.values():
                        reg.set_mode(self._fine_mode)
            self._packed = (ncn, mid, fine)
        return self._packed

    def set_coarse_mode(self, mode):
        """'fp16x2' (default, fp32-equivalent) or the opt-in 'fp16' for the matrix-core kernels of the coarse stage (one fp16
        plane per operand, one MFMA product per product: NOT fp32-equivalent, see ops.NcnWeights.set_mode).  The choice belongs
        to the model: it is applied to the packed consensus handle now and again whenever the weights are re-packed
        (load_state_dict, init_weights_).  A model with a generic consensus stack (any but the released one) accepts 'generic'
        (default, exact fp32 MFMA) and the opt-in 'generic_fp16x2' (fp32-equivalent, ops.NcnWeights.set_mode) instead.  A name of
        the other kind raises NotImplementedError, an unknown one ValueError -- both before anything changes."""
        generic = self._ncn_layout != ops.RELEASED_NCN_LAYOUT
        names = ops._lib.COARSE_MODES_GENERIC if generic else ops._lib.COARSE_MODES
        if not isinstance(mode, str) or (mode not in ops._lib.COARSE_MODES and mode not in ops._lib.COARSE_MODES_GENERIC):
            raise ValueError(f"unknown coarse mode {mode!r}: one of {sorted(names)}")
        if mode not in names:
            raise NotImplementedError(f"set_coarse_mode: {mode!r} is no mode of this model's consensus stack (one of {sorted(names)})")
        self._coarse_mode = mode
        if self._packed is not None:
            self._packed[0].set_mode(mode)

    @property
    def coarse_mode(self):
        """The mode `set_coarse_mode` chose, or the one new handles start in (P2P_COARSE_MODE, else 'fp16x2'); for a generic
        consensus stack the chosen generic name, P2P_COARSE_GENERIC_MODE=generic_fp16x2 when set, else 'fp16x2' as before."""
        if self._ncn_layout != ops.RELEASED_NCN_LAYOUT:
            start = ops.default_coarse_generic_mode()
            return getattr(self, "_coarse_mode", None) or (start if start != "generic" else "fp16x2")
        return getattr(self, "_coarse_mode", None) or ops.default_coarse_mode()

    def _fine_mode_names(self):
        """The mode names the packed regressors of this model accept: the generic ones for a generic regressor, the tuned ones
        for the released configuration."""
        if self._layout != ops.RELEASED_LAYOUT:
            return dict(ops._lib.REGRESS_MODES_GENERIC)
        return {**ops._lib.REGRESS_MODES, **ops._lib.REGRESS_MODES_LOSSY}

    def set_fine_mode(self, mode):
        """The arithmetic of the fine stage's convolutions (ops.RegressorWeights.set_mode).  A model with generic regressors (any
        configuration but the released one) accepts 'generic' (default, exact fp32 MFMA) and the opt-in 'generic_fp16x2' (two fp16
        planes per operand, three MFMA products, fp32-equivalent); a model with the released configuration accepts the tuned names
        ('fp16x2w', 'fp16x2', 'f32', the opt-in lossy 'fp16').  A name of the other kind raises NotImplementedError, an unknown one
        ValueError, a model without regressors ValueError -- all before anything changes.  The choice belongs to the model: it is
        applied to both packed handles now and again whenever the weights are re-packed (load_state_dict, init_weights_)."""
        if self.regress_mid is None:
            raise ValueError("set_fine_mode: this model has no regressors")
        known = {**ops._lib.REGRESS_MODES, **ops._lib.REGRESS_MODES_LOSSY, **ops._lib.REGRESS_MODES_GENERIC}
        if mode not in known:
            raise ValueError(f"unknown fine mode {mode!r}: one of {sorted(self._fine_mode_names())}")
        if mode not in self._fine_mode_names():
            raise NotImplementedError(f"set_fine_mode: {mode!r} is no mode of this model's regressors "
                                      f"(one of {sorted(self._fine_mode_names())})")
        self._fine_mode = mode
        if self._packed is not None:
            for reg in {id(r): r for r in self._packed[1:]}.values():
                reg.set_mode(mode)

    @property
    def fine_mode(self):
        """The mode `set_fine_mode` chose, or the one new handles start in (P2P_REGRESS_GENERIC_MODE, else 'generic', for generic
        regressors; P2P_REGRESS_MODE, else 'fp16x2w', for the released configuration); None for a model without regressors."""
        if self.regress_mid is None:
            return None
        chosen = getattr(self, "_fine_mode", None)
        if chosen is not None:
            return chosen
        if self._layout != ops.RELEASED_LAYOUT:
            return os.environ.get("P2P_REGRESS_GENERIC_MODE") or "generic"
        return os.environ.get("P2P_REGRESS_MODE") or "fp16x2w"

    # ------------------------------------------------------------------ coarse stage
    def forward_coarse_match(self, feat1, feat2, ksize=1):
        ncn = self._weights()[0]
        b, _, h1, w1 = feat1.shape
        _, _, h2, w2 = feat2.shape
        k = max(ksize, 1)
        shape = (b, 1, h1 // k, w1 // k, h2 // k, w2 // k)
        corr4d = torch.empty(shape, dtype=torch.float32, device=feat1.device)
        packed = torch.empty(shape, dtype=torch.uint8, device=feat1.device) if ksize > 1 else None
        ops.coarse_forward_batch(feat1, feat2, ksize, ncn, out_corr=corr4d[:, 0],
                                 out_delta=packed[:, 0] if packed is not None else None)
        delta4d = Delta4d(packed[:, 0], ksize) if ksize > 1 else None
        return corr4d, delta4d

    def forward(self, im1, im2, ksize=1, return_feats=False):
        feat1s, feat2s = self._pyramids(im1, im2)
        feat1, feat2 = feat1s[-1], feat2s[-1]
        corr4d, delta4d = self.forward_coarse_match(feat1, feat2, ksize=ksize)
        if return_feats:
            return corr4d, delta4d, feat1s, feat2s
        return corr4d, delta4d

    def _packed_delta(self, delta4d, ksize):
        if delta4d is not None and not isinstance(delta4d, Delta4d):
            di, dj, dk, dl = delta4d            # reference-format int64 planes -> packed byte
            s = ((di * ksize + dj) * ksize + dk) * ksize + dl
            delta4d = Delta4d(s[:, 0].to(torch.uint8).contiguous(), ksize)
        return delta4d.packed if delta4d is not None else None

    def cal_coarse_matches(self, corr4d, delta4d, ksize=1, do_softmax=True, upsample=16, sort=False,
                           center=True, pshift=0):
        packed = self._packed_delta(delta4d, ksize)
        if do_softmax:
            matches_, score_ = ops.coarse_matches_batch(corr4d[:, 0], packed, ksize, upsample, center)
        else:       # raw consensus values as scores: the top-k entry with one candidate per cell
            matches_, score_ = ops.coarse_matches_topk_batch(corr4d[:, 0], packed, ksize, upsample, center, 1, False)
        if sort:
            order = torch.sort(-score_)[1]
            score_ = torch.gather(score_, 1, order)
            matches_ = torch.gather(matches_, 1, order.unsqueeze(-1).expand(-1, -1, 4))
        return matches_, score_

    def cal_coarse_matches_topk(self, corr4d, delta4d, topk, ksize=1, do_softmax=True, upsample=16, center=True):
        """cal_coarse_matches with the `topk` best candidates per cell and direction (corr_to_matches_topk,
        ncn/extract_ncmatches.py:96-158, in both directions): ([B,topk*(nB+nA),4] int64, [B,topk*(nB+nA)] fp32); rank t of
        B cell c in row t*nB + c, rank t of A cell r in row topk*nB + r*topk + t; ties by ascending cell index."""
        return ops.coarse_matches_topk_batch(corr4d[:, 0], self._packed_delta(delta4d, ksize), ksize, upsample, center,
                                             topk, do_softmax)

    def cal_coarse_score(self, corr4d, normalize='softmax'):
        """patch2pix.py:320-338: the NCNet pair score of corr4d [B,1,h1,w1,h2,w2] -- the mean over all cells of both images
        (and over the batch) of the best normalised consensus value; normalize None, 'softmax' or 'l1'.  A 0-dim tensor on
        the device: the fp32 mean of the B per-pair scores (every pair of a batch has the same cell count).  Any other
        `normalize` raises ValueError."""
        return ops.coarse_score_batch(corr4d[:, 0], normalize).mean()

    def score_from_feats(self, feats1, feats2, ksize=2, normalize='softmax'):
        """One score per pair from one coarse stage (non-reference): [B] fp32 on the device, cal_coarse_score of every pair
        on its own, with no match extraction and no fine stage.  feats*: the pyramids (or any sequence whose last entry
        is the [B,C,h,w] coarse feature map)."""
        ops.score_norm(normalize)                  # a bad value raises before the coarse stage is paid for
        corr4d, _ = self.forward_coarse_match(feats1[-1], feats2[-1], ksize=ksize)
        return ops.coarse_score_batch(corr4d[:, 0], normalize)

    def predict_score(self, im1, im2, ksize=2, normalize='softmax'):
        """score_from_feats from the images: the call a re-ranking loop makes per shortlist batch."""
        ops.score_norm(normalize)
        feats1, feats2 = self._pyramids(im1, im2)
        return self.score_from_feats(feats1, feats2, ksize, normalize)

    def shift_to_anchors(self, matches):
        """patch2pix.py:377-402: panc == 8 replaces each match by its 8 corner-shifted anchors."""
        if self.panc == 1:
            return matches
        s = self.pshift
        tmpl = torch.tensor([[-s, -s, 0, 0], [s, -s, 0, 0], [-s, s, 0, 0], [s, s, 0, 0],
                             [0, 0, -s, -s], [0, 0, s, -s], [0, 0, -s, s], [0, 0, s, s]], device=self.device)
        return [(m.unsqueeze(1) + tmpl).reshape(-1, 4) for m in matches]

    # ------------------------------------------------------------------ fine stage
    def forward_fine_match(self, feats1, feats2, coarse_matches, psize=16, ptype="center", regressor=None):
        """One regressor over every batch item (reference patch2pix.py:186-218).  `regressor` is
        `self.regress_mid` / `self.regress_fine` like in the reference call sites."""
        _, mid_w, fine_w = self._weights()
        w = fine_w if (regressor is self.regress_fine and regressor is not self.regress_mid) else mid_w
        nb = len(coarse_matches)
        outs = ops.regress_batch(w, None, [[f[b] for f in feats1[:4]] for b in range(nb)],
                                 [[f[b] for f in feats2[:4]] for b in range(nb)],
                                 [self._as_proposals(p) for p in coarse_matches])
        return [o["matches1"] for o in outs], [o["probs1"] for o in outs]

    def _as_proposals(self, props):
        props = props.to(self.device)
        if props.dtype not in (torch.int64, torch.float32):
            props = props.float() if props.is_floating_point() else props.long()
        return props

    def _fine_chain(self, feats1, feats2, coarse_matches):
        """mid -> fine for every batch item in one launch each (patch2pix.py:259-272)."""
        _, mid_w, fine_w = self._weights()
        nb = len(coarse_matches)
        outs = ops.regress_batch(mid_w, fine_w, [[f[b] for f in feats1[:4]] for b in range(nb)],
                                 [[f[b] for f in feats2[:4]] for b in range(nb)],
                                 [self._as_proposals(p) for p in coarse_matches])
        return ([o["matches2"] for o in outs], [o["probs2"] for o in outs],
                [o["matches1"] for o in outs], [o["probs1"] for o in outs])

    # ------------------------------------------------------------------ public prediction API
    def predict_coarse(self, im1, im2, ksize=2, ncn_thres=0.0, mutual=False, center=True):
        corr4d, delta4d = self.forward(im1, im2, ksize)
        coarse_matches, match_scores = self.cal_coarse_matches(corr4d, delta4d, ksize=ksize,
                                                               upsample=self.upsample, center=center)
        return filter_coarse(coarse_matches, match_scores, ncn_thres, mutual)

    def predict_coarse_topk(self, im1, im2, topk, ksize=2, ncn_thres=0.0, mutual=False, center=True):
        """predict_coarse over `topk` candidates per cell and direction."""
        corr4d, delta4d = self.forward(im1, im2, ksize)
        coarse_matches, match_scores = self.cal_coarse_matches_topk(corr4d, delta4d, topk, ksize=ksize,
                                                                    upsample=self.upsample, center=center)
        return filter_coarse(coarse_matches, match_scores, ncn_thres, mutual)

    def predict_fine_topk(self, im1, im2, topk, ksize=2, ncn_thres=0.0, mutual=True, return_all=False):
        """predict_fine over `topk` candidates per cell and direction: k times the proposals from one coarse stage, each
        scored by the regressors (host-side filter_coarse; same return layout as predict_fine)."""
        feats1, feats2 = self._pyramids(im1, im2)
        corr4d, delta4d = self.forward_coarse_match(feats1[-1], feats2[-1], ksize=ksize)
        matches_, score_ = self.cal_coarse_matches_topk(corr4d, delta4d, topk, ksize=ksize, upsample=self.upsample,
                                                        center=True)
        coarse_matches, _ = filter_coarse(matches_, score_, ncn_thres, mutual)
        coarse_matches = self.shift_to_anchors(coarse_matches)
        fine, fine_scores, mid, mid_scores = self._fine_chain(feats1, feats2, coarse_matches)
        if return_all:
            return fine, fine_scores, mid, mid_scores, coarse_matches
        return fine, fine_scores, coarse_matches

    def coarse_async(self, feats1, feats2, ksize=2):
        """Enqueue the coarse stage of a batch and an asynchronous device-to-host copy of its
        (small) match arrays behind it; returns a ticket for `fine_from_ticket`.  Lets a
        caller enqueue the next batch's coarse stage before it filters the current one on the host,
        so that the host-side filter_coarse (reference networks/utils.py:38-72) never idles the GPU."""
        corr4d, delta4d = self.forward_coarse_match(feats1[-1], feats2[-1], ksize=ksize)
        matches_, score_ = self.cal_coarse_matches(corr4d, delta4d, ksize=ksize, upsample=self.upsample, center=True)
        # The copies go to the stream that produced the arrays, in front of whatever the caller enqueues next: the
        # regress launch is one persistent work-group per compute unit, so a copy kernel on a side stream that becomes
        # ready when that launch has started would wait for its end (17 ms at 6400 proposals) -- and the host with it.
        # A fifth ticket while the first is still pending takes over its staging slot: the old ticket then falls back
        # to its own device-to-host copy when (if) it is consumed.
        return dict(feats1=feats1, feats2=feats2, matches=matches_, scores=score_,
                    staged=staging.readback([matches_, score_], self._ticket_ring))

    def fine_from_ticket(self, ticket, ncn_thres=0.0, mutual=True, return_all=False, ptmax=None):
        host = ticket["staged"].wait()          # None: the staging slot went to a later ticket
        coarse_matches, match_scores = filter_coarse(ticket["matches"], ticket["scores"], ncn_thres, mutual, ptmax=ptmax,
                                                     host_copy=None if host is None else (host[0].numpy(), host[1].numpy()))
        coarse_matches = self.shift_to_anchors(coarse_matches)
        fine, fine_scores, mid, mid_scores = self._fine_chain(ticket["feats1"], ticket["feats2"], coarse_matches)
        if return_all:
            return fine, fine_scores, mid, mid_scores, coarse_matches
        return fine, fine_scores, coarse_matches

    def predict_fine_device(self, feats1, feats2, ksize=2, ncn_thres=0.0, mutual=True):
        """The whole path without a host round trip: coarse stage -> device-side filter_coarse -> both
        regressors reading the proposal counts from device memory.  Returns padded device tensors
        (fine [B,n,4], fine_scores [B,n], coarse [B,n,4] int64, counts int32 [B]); `unpad` turns them into the lists
        predict_fine returns.  Not available for the training-time options (ptmax, panc > 1) and for images whose pixel
        coordinates do not fit 15 bits -- use predict_fine_from_feats there.  Any number of coarse rows up to 2^20 per
        pair (lists beyond the 8192 rows that fit LDS are sorted through a scratch buffer, csrc/filter.hip)."""
        if self.panc != 1:
            raise NotImplementedError("predict_fine_device: panc > 1 goes through predict_fine_from_feats")
        if max(feats1[0].shape[-2:] + feats2[0].shape[-2:]) >= (1 << 15):
            raise NotImplementedError("predict_fine_device: image sides must be below 32768 pixels")
        _, mid_w, fine_w = self._weights()
        corr4d, delta4d = self.forward_coarse_match(feats1[4], feats2[4], ksize=ksize)
        matches_, score_ = self.cal_coarse_matches(corr4d, delta4d, ksize=ksize, upsample=self.upsample, center=True)
        coarse, _, counts = ops.filter_coarse_batch(matches_, score_, ncn_thres, mutual)
        nb = coarse.shape[0]
        out = ops.regress_batch_dev(mid_w, fine_w, [[f[b] for f in feats1[:4]] for b in range(nb)],
                                    [[f[b] for f in feats2[:4]] for b in range(nb)], coarse, counts)
        return out["matches2"], out["probs2"], coarse, counts

    @staticmethod
    def unpad(fine, fine_scores, coarse, counts):
        """One device-to-host copy of the counts, then per-item views: the (fine, scores, coarse) lists of predict_fine.
        A count of -1 (the device filter met a coordinate outside its packed key) raises: the padded rows of that item
        hold nothing, use predict_fine_from_feats for such inputs."""
        n = counts.cpu().tolist()
        if any(c < 0 for c in n):
            raise RuntimeError("Patch2Pix.unpad: the device-side filter_coarse asked for the host path (count -1: a "
                               "coordinate outside [0, 2^15)); call predict_fine_from_feats / estimate_matches instead")
        return ([fine[b, :c] for b, c in enumerate(n)], [fine_scores[b, :c] for b, c in enumerate(n)],
                [coarse[b, :c] for b, c in enumerate(n)])

    def predict_fine_from_feats(self, feats1, feats2, ksize=2, ncn_thres=0.0, mutual=True, return_all=False,
                                ptmax=None):
        """predict_fine after the backbone: the part of the path that is HIP end to end.
        `ptmax` (opt-in, training semantics of utils.py:55-63) caps/tiles the proposals."""
        ticket = self.coarse_async(feats1, feats2, ksize)
        return self.fine_from_ticket(ticket, ncn_thres, mutual, return_all, ptmax)

    def _pyramids(self, im1, im2):
        return resnet.pair_pyramids(self.extract, im1, im2)

    def predict_fine(self, im1, im2, ksize=2, ncn_thres=0.0, mutual=True, return_all=False):
        feats1, feats2 = self._pyramids(im1, im2)
        return self.predict_fine_from_feats(feats1, feats2, ksize, ncn_thres, mutual, return_all)

    def refine_matches(self, im1, im2, coarse_matches, io_thres):
        """patch2pix.py:278-318: refine caller-supplied coarse matches (numpy or tensor [N,4])."""
        if len(coarse_matches) == 0:
            return np.empty((0, 4)), np.empty((0,)), np.empty((0, 4))
        if isinstance(coarse_matches, np.ndarray):
            coarse_t = torch.from_numpy(coarse_matches).to(self.device)
        else:
            coarse_t = coarse_matches.to(self.device)
            coarse_matches = coarse_matches.cpu().data.numpy()
        feats1, feats2 = self._pyramids(im1, im2)
        fine, fine_scores, _, _ = self._fine_chain(feats1, feats2, [coarse_t])
        refined = fine[0].cpu().data.numpy()
        scores = fine_scores[0].cpu().data.numpy()
        if io_thres > 0:
            pos = np.where(scores > io_thres)[0]
            if len(pos) > 0:
                coarse_matches, refined, scores = coarse_matches[pos], refined[pos], scores[pos]
        return refined, scores, coarse_matches
