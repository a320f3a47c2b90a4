"""No GPU: backbone names, strides and the feat_idx rule of Patch2Pix(config); state-dict keys of ResNet50 / ResNet101 against the
reference's own modules; the torch path against the reference's forward_all; the cache signature of a Bottleneck trunk; the
seeded checkpoints."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bottleneck_reference as br  # noqa: E402
from oracle import ref_shim  # noqa: E402
from patch2pix_amd.networks import patch2pix, resnet  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="the reference tree is not on this machine")


@pytest.mark.parametrize("backbone,dims", [("ResNet34", [3, 64, 64, 128, 256]), ("ResNet50", [3, 64, 256, 512, 1024]),
                                           ("ResNet101", [3, 64, 256, 512, 1024])])
@pytest.mark.parametrize("change_stride", [True, False])
def test_names_and_strides(backbone, dims, change_stride):
    cls, upsample, down = patch2pix.backbone_layout(backbone, change_stride)
    assert cls is getattr(resnet, backbone)
    assert upsample == (8 if change_stride else 16) and down == [1, 2, 2, 2, 1 if change_stride else 2]
    net = cls()
    if change_stride:
        net.change_stride("layer3")
    assert net.feat_dims == dims
    with torch.no_grad():
        feats = net.eval().pyramid(torch.randn(1, 3, 32, 48))
    assert [f.shape[1] for f in feats] == dims
    assert tuple(feats[3].shape[-2:]) == (4, 6) and tuple(feats[4].shape[-2:]) == ((4, 6) if change_stride else (2, 3))


def test_unknown_backbone_and_feat_idx_rule():
    for bad in ("ResNet18", "ResNet152", "resnet50", ""):
        with pytest.raises(NotImplementedError, match="ResNet34, ResNet50, ResNet101"):
            patch2pix.backbone_layout(bad, True)
    for backbone in ("ResNet50", "ResNet101"):
        for ok in ([0], [1], [0, 1]):
            patch2pix.backbone_layout(backbone, True, ok)
        for fi, lvl, ch in (([0, 1, 2], 2, 256), ([3], 3, 512), ([1, 4], 4, 1024), ([0, 1, 2, 3], 2, 256)):
            with pytest.raises(ValueError, match=f"level {lvl} of a {backbone} pyramid has {ch} channels"):
                patch2pix.backbone_layout(backbone, False, fi)
    patch2pix.backbone_layout("ResNet34", False, [0, 1, 2, 3])
    patch2pix.backbone_layout("ResNet34", True, [0, 1, 2, 3, 4])          # level 4 is the fine stage's own refusal (ops.regressor_layout)


def _config(backbone, regressor, feat_idx, change_stride=True):
    from argparse import Namespace
    rc = br.regressor_config(regressor)
    return Namespace(training=False, device="cuda", regr_batch=1200, backbone=backbone, feat_idx=feat_idx, weights_dict=None,
                     regressor_config=rc, change_stride=change_stride)


def test_constructor_applies_the_rules(monkeypatch):
    """Patch2Pix(config) itself, not only the helper: a bad name or a bad feat_idx raises before anything touches a device, and
    feat_idx reaches the rule exactly when the model has regressors (an NC-only model may carry any feat_idx, like the
    reference's, which never reads it then)."""
    for bad in ("ResNet18", "resnet50"):
        with pytest.raises(NotImplementedError, match="ResNet34, ResNet50, ResNet101"):
            patch2pix.Patch2Pix(_config(bad, None, None))
    for backbone in ("ResNet50", "ResNet101"):
        for cs in (True, False):
            with pytest.raises(ValueError, match=f"level 2 of a {backbone} pyramid has 256 channels"):
                patch2pix.Patch2Pix(_config(backbone, "released", [0, 1, 2, 3], cs))
        with pytest.raises(ValueError, match=f"level 3 of a {backbone} pyramid has 512 channels"):
            patch2pix.Patch2Pix(_config(backbone, "small", [1, 3]))

    class Reached(Exception):
        pass
    seen = []

    def spy(backbone, change_stride, feat_idx=None):
        seen.append((backbone, change_stride, feat_idx))
        raise Reached()
    monkeypatch.setattr(patch2pix, "backbone_layout", spy)
    with pytest.raises(Reached):
        patch2pix.Patch2Pix(_config("ResNet50", None, [0, 1, 2, 3], False))      # NC-only: the levels are nobody's business
    with pytest.raises(Reached):
        patch2pix.Patch2Pix(_config("ResNet50", "small", [0, 1], True))
    with pytest.raises(Reached):
        patch2pix.Patch2Pix(_config("ResNet34", "released", [0, 1, 2, 3], False))
    assert seen == [("ResNet50", False, None), ("ResNet50", True, [0, 1]), ("ResNet34", False, [0, 1, 2, 3])]


@needs_reference
@pytest.mark.parametrize("backbone", ["ResNet50", "ResNet101"])
def test_state_dict_keys_equal_the_reference(backbone):
    ref = ref_shim.load_reference()
    theirs = {k: tuple(v.shape) for k, v in getattr(ref.resnet, backbone)().state_dict().items() if not k.startswith("layer4.")}
    ours = {k: tuple(v.shape) for k, v in getattr(resnet, backbone)().state_dict().items()}
    assert ours == theirs
    sd = synthetic.make_backbone_checkpoint(3, backbone)["state_dict"]
    made = {k[len("extract."):]: tuple(v.shape) for k, v in sd.items() if k.startswith("extract.")}
    assert made == theirs


@needs_reference
@pytest.mark.parametrize("backbone,change_stride", [("ResNet50", True), ("ResNet50", False), ("ResNet101", True), ("ResNet34", False)])
def test_torch_path_equals_the_reference_forward_all(backbone, change_stride):
    ref = ref_shim.load_reference()
    sd = {k[len("extract."):]: v for k, v in synthetic.make_backbone_checkpoint(4, backbone, change_stride)["state_dict"].items()
          if k.startswith("extract.")}
    ours, theirs = getattr(resnet, backbone)(), getattr(ref.resnet, backbone)()
    ours.load_state_dict(sd)
    theirs.load_state_dict(sd, strict=False)           # its layer4 keeps its initial values: never used
    if change_stride:
        ours.change_stride("layer3"); theirs.change_stride("layer3")
    x = torch.randn(2, 3, 48, 80)
    want = []
    with torch.no_grad():
        theirs.eval().forward_all(x, want, early_feat=True)
        got = ours.eval().pyramid(x)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_checkpoint_maker():
    a = synthetic.make_backbone_checkpoint(11, "ResNet50", False)
    b = synthetic.make_backbone_checkpoint(11, "ResNet50", False)
    assert a["backbone"] == "ResNet50" and a["change_stride"] is False and a["regressor_config"] is None
    assert all(torch.equal(a["state_dict"][k], v) for k, v in b["state_dict"].items())
    sd = a["state_dict"]
    assert not any(k.startswith("regress_") for k in sd) and "ncn.conv.0.weight" in sd
    bn = "extract.layer3.5.bn3"
    assert float(sd[bn + ".running_var"].std()) > 0 and float(sd[bn + ".running_mean"].abs().max()) > 0      # BatchNorm is no no-op
    c = synthetic.make_backbone_checkpoint(12, "ResNet50", True, br.regressor_config("small"), [0, 1])
    assert tuple(c["state_dict"]["regress_mid.conv.0.weight"].shape) == (64, 2 * 67, 3, 3) and c["feat_idx"] == [0, 1]
    shift = torch.full((1024,), 0.25)
    d = synthetic.make_backbone_checkpoint(11, "ResNet50", False, contrast=shift)["state_dict"]
    assert torch.equal(d[bn + ".bias"], sd[bn + ".bias"] - shift)
    assert synthetic.make_state_dict(0).keys() == synthetic.make_checkpoint(0)["state_dict"].keys()


def test_hip_signature_sees_a_bottleneck_weight():
    net = resnet.ResNet50().eval()
    sig = net._hip_signature("cpu")
    assert len(sig) == 1 + 6 * (1 + 3 * 13 + 3)            # 5 tensors + the stride of the stem, 39 block convolutions, 3 projections
    with torch.no_grad():
        net.layer2[1].conv3.weight.mul_(2.0)
    sig2 = net._hip_signature("cpu")
    assert sig2 != sig
    with torch.no_grad():
        net.layer3[5].bn3.running_var.add_(1.0)
    assert net._hip_signature("cpu") != sig2
    net.change_stride("layer3")
    assert net._hip_signature("cpu")[-1] == (1, 1) and net.layer3[0].conv1.stride == (1, 1) and net.layer3[0].conv2.stride == (1, 1)
