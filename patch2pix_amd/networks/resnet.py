"""Feature-pyramid producer for the matching hot path.

Role of reference networks/resnet.py:125-191 (ResNet34, ResNet50 and ResNet101 truncated after layer3, with or without the
layer3 stride patch of `change_stride`), SURVEY.md section 8 row f1.  The module keeps the torch
parameters (checkpoints load unchanged); on the GPU in eval mode the convolutions of
stem and of layer1..layer3 (32 for ResNet34, 43 for ResNet50, 94 for ResNet101) run as the library's fp32-equivalent fp16 MFMA kernels (csrc/backbone.hip;
NHWC activations between the layers, NCHW pyramid levels out), the max-pool as its own kernel.
`P2P_BACKBONE=miopen` selects the all-PyTorch path (the round-1/2 producer).  Parameter names follow the torchvision ResNet convention so that
reference checkpoints (`extract.*` keys, utils/train/helper.py:10-17) load unchanged;
`layer4.*` keys of a checkpoint are never used by the path (reference
networks/patch2pix.py:72-74 freezes them as "never used") and are skipped on load.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

# (planes, blocks, stride of first block) up to layer3
_STAGES = (("layer1", 64, 3, 1), ("layer2", 128, 4, 2), ("layer3", 256, 6, 2))                  # ResNet34, ResNet50
_STAGES101 = (("layer1", 64, 3, 1), ("layer2", 128, 4, 2), ("layer3", 256, 23, 2))


class _Basic(nn.Module):
    """Two 3x3 conv+BN with identity / projected skip."""

    expansion = 1
    convs = (("conv1", "bn1"), ("conv2", "bn2"))       # in the order they run; the last one takes the skip

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False),
                                            nn.BatchNorm2d(cout))

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)), inplace=True)
        y = self.bn2(self.conv2(y))
        return F.relu(y + skip, inplace=True)


class _Bottleneck(nn.Module):
    """1x1 -> 3x3 (carries the stride) -> 1x1 to 4 x planes, conv+BN each, with identity / projected skip
    (reference resnet.py:49-85)."""
    expansion = 4
    convs = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))

    def __init__(self, cin, planes, stride):
        super().__init__()
        cout = planes * self.expansion
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False),
                                            nn.BatchNorm2d(cout))

    def forward(self, x):
        skip = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)), inplace=True)
        y = F.relu(self.bn2(self.conv2(y)), inplace=True)
        y = self.bn3(self.conv3(y))
        return F.relu(y + skip, inplace=True)


class _ResNet(nn.Module):
    """conv1/bn1 + layer1..layer3 of a ResNet; `pyramid()` returns the 5 maps the path reads.  The three backbones below differ
    in the two class attributes only."""
    block, stages = None, None

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for name, planes, blocks, stride in self.stages:
            cout = planes * self.block.expansion
            seq = [self.block(cin, planes, stride)] + [self.block(cout, planes, 1) for _ in range(blocks - 1)]
            setattr(self, name, nn.Sequential(*seq))
            cin = cout
        self.feat_dims = [3, 64] + [planes * self.block.expansion for _, planes, _, _ in self.stages]

    def change_stride(self, target="layer3"):
        """Make `target`'s first block stride-1 (reference resnet.py:169-173, literally: conv1, conv2 and downsample[0] -- in a
        Bottleneck block conv1 is stride 1 already)."""
        blk = getattr(self, target)[0]
        for conv in (blk.conv1, blk.conv2, blk.downsample[0]):
            conv.stride = (1, 1)

    def __getstate__(self):
        """copy.deepcopy / pickling: the packed device-side weights are a cache, not part of the module."""
        state = self.__dict__.copy()
        state.pop("_hip_trunk_cache", None)
        state.pop("_hip_sig", None)
        return state

    def _hip_signature(self, device):
        """(device, identity, version counter and storage of every tensor the packed weights were made from): changes with
        load_state_dict / in-place edits (version), .to() / .data assignment (storage) and replaced Parameter objects
        (identity).  Walks the known structure through the modules' own dictionaries: the generic parameters() /
        buffers() iterators cost a millisecond per call, more than launching the 36 kernels."""
        sig = [str(device)]
        pairs = [(self.conv1, self.bn1)]
        for name, _, _, _ in self.stages:
            for blk in self._modules[name]._modules.values():
                m = blk._modules
                pairs += [(m[c], m[b]) for c, b in self.block.convs]
                if m.get("downsample") is not None:
                    d = m["downsample"]._modules
                    pairs.append((d["0"], d["1"]))
        for conv, bn in pairs:
            for t in (conv._parameters["weight"], bn._parameters["weight"], bn._parameters["bias"],
                      bn._buffers["running_mean"], bn._buffers["running_var"]):
                sig.append((id(t), t._version, t.data_ptr()))
            sig.append(conv.stride)
        return tuple(sig)

    def _hip_trunk(self, device):
        """The packed convolutions of layer1..layer3 for `device`, re-packed when a parameter changed."""
        from .. import ops
        sig = self._hip_signature(device)
        if getattr(self, "_hip_sig", None) != sig:
            def pack(conv, bn):
                if abs(bn.eps - 1e-5) > 1e-12:      # the packed BatchNorm fold uses the reference's eps (resnet.py: nn.BatchNorm2d default)
                    raise NotImplementedError(f"BatchNorm eps {bn.eps}: the HIP pyramid producer folds eps = 1e-5 (set P2P_BACKBONE=miopen)")
                return ops.ConvBN(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.stride[0], device)
            trunk = []
            for name, _, _, _ in self.stages:
                blocks = []
                for blk in getattr(self, name):
                    down = pack(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None
                    # (the block's convolutions in the order they run ..., its projection or None)
                    blocks.append(tuple(pack(getattr(blk, c), getattr(blk, b)) for c, b in blk.convs) + (down,))
                trunk.append(blocks)
            if abs(self.bn1.eps - 1e-5) > 1e-12:
                raise NotImplementedError(f"BatchNorm eps {self.bn1.eps}: the HIP pyramid producer folds eps = 1e-5 (set P2P_BACKBONE=miopen)")
            stem = ops.Stem(self.conv1.weight, self.bn1.weight, self.bn1.bias, self.bn1.running_mean, self.bn1.running_var, device)
            self._hip_trunk_cache, self._hip_sig = (stem, trunk), sig
            if getattr(self, "_hip_mode", None) is not None:       # the new handles start in the default mode
                self._apply_hip_mode()
        return self._hip_trunk_cache

    def _apply_hip_mode(self):
        stem, trunk = self._hip_trunk_cache
        stem.set_mode(self._hip_mode)
        for blocks in trunk:
            for layers in blocks:
                for layer in layers:
                    if layer is not None:
                        layer.set_mode(self._hip_mode)

    def set_mode(self, mode):
        """Arithmetic of the HIP pyramid producer, every packed layer: 'fp16x2' (default, fp32-equivalent) or the opt-in 'fp16'
        (one fp16 plane per operand, one MFMA product per product: NOT fp32-equivalent, see ops.ConvBN.set_mode).  The choice
        belongs to the module: it survives the re-pack after load_state_dict / .to().  The torch path (P2P_BACKBONE=miopen,
        train(), non-fp32 input) does not look at it.  Must not race with a forward on another stream or thread; a captured
        graph keeps the arithmetic it was captured with."""
        from .. import ops
        ops.backbone_mode_id(mode)                                  # ValueError for an unknown name, before anything changes
        self._hip_mode = mode
        if getattr(self, "_hip_trunk_cache", None) is not None:
            self._apply_hip_mode()

    @property
    def mode(self):
        """The mode `set_mode` chose, or the one new handles start in (P2P_BACKBONE_MODE, else 'fp16x2')."""
        from .. import ops
        return getattr(self, "_hip_mode", None) or ops.default_backbone_mode()

    def _pyramid_hip(self, x):
        # every launch below goes to the current stream of the CURRENT device: make the input's device current (a model on
        # cuda:1 driven from a process whose current device is cuda:0 would otherwise launch there with device-1 pointers)
        with torch.cuda.device(x.device):
            return self._pyramid_hip_on_current_device(x)

    def _pyramid_hip_on_current_device(self, x):
        from .. import ops
        stem, trunk = self._hip_trunk(x.device)
        feats = [x]
        x = stem.forward(x)
        feats.append(x)
        # float bits of max |activation| per image, one row per layer output: raised by the producing kernel (atomicMax)
        per_block = len(self.block.convs)
        maxima = torch.zeros((1 + per_block * sum(len(b) for b in trunk), x.shape[0]), device=x.device, dtype=torch.int32)
        xmax, row = maxima[0], 1
        x = ops.maxpool_nhwc(x, xmax)                                          # NHWC from here on
        for blocks in trunk:
            for *convs, down in blocks:
                # the projection without ReLU; ReLU after every convolution, the last one behind the residual
                skip = x if down is None else down.forward(x, xmax, relu=False)
                y, ymax = x, xmax
                for conv in convs[:-1]:
                    y = conv.forward(y, ymax, ymax=maxima[row])
                    ymax, row = maxima[row], row + 1
                x = convs[-1].forward(y, ymax, residual=skip, ymax=maxima[row])
                xmax, row = maxima[row], row + 1
            feats.append(ops.nhwc_to_nchw(x))
        return feats

    def pyramid(self, x):
        """[image, relu(bn1(conv1)), layer1, layer2, layer3] -- reference forward_all (resnet.py:138-157)."""
        # the HIP producer: fp32 inference only -- a half / double image, or one autograd has to flow through, takes the torch path
        if (x.is_cuda and not self.training and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad)
                and os.environ.get("P2P_BACKBONE", "hip") != "miopen"):
            return self._pyramid_hip(x)
        feats = [x]
        x = F.relu(self.bn1(self.conv1(x)), inplace=True)
        feats.append(x)
        x = self.layer1(F.max_pool2d(x, 3, 2, 1))
        feats.append(x)
        x = self.layer2(x)
        feats.append(x)
        x = self.layer3(x)
        feats.append(x)
        return feats

    def forward_all(self, x, feat_list=None, early_feat=True):
        """Reference-compatible signature: appends the pyramid to `feat_list`."""
        feats = self.pyramid(x)
        if feat_list is not None:
            feat_list.extend(feats)
        return feats

    def forward(self, x, early_feat=True):
        return self.pyramid(x)[-1]


class ResNet34(_ResNet):
    """BasicBlock (3, 4, 6): 64 / 64 / 128 / 256 channels at levels 1..4, the released model (reference resnet.py:175-179)."""
    block, stages = _Basic, _STAGES


class ResNet50(_ResNet):
    """Bottleneck blocks (3, 4, 6): 64 / 256 / 512 / 1024 channels at levels 1..4 (reference resnet.py:181-185)."""
    block, stages = _Bottleneck, _STAGES


class ResNet101(_ResNet):
    """Bottleneck blocks (3, 4, 23): the backbone NCNet was published with (reference resnet.py:187-191)."""
    block, stages = _Bottleneck, _STAGES101


def pair_pyramids(extract, im1, im2, both=None):
    """The pyramids of two image batches; equally sized ones go through the backbone as one batch (an image's pyramid
    does not depend on its batch mates: tests/test_gpu_parity.py::test_backbone_batch_and_tile_independence).  `both`:
    the tensor `im1` and `im2` are the halves of, where the caller has it (saves the concatenation)."""
    if both is None and im1.shape == im2.shape:
        both = torch.cat([im1, im2])
    if both is None:
        return extract.pyramid(im1), extract.pyramid(im2)
    feats, n = extract.pyramid(both), im1.shape[0]
    return [f[:n] for f in feats], [f[n:] for f in feats]
