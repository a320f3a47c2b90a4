"""Backbone mode 'fp16' (P2P_CONV_FP16) on the MI355X through the real library: the element-wise bounds, tile / batch / default
equalities of tests/test_backbone_mode_emulated.py on ops.ConvBN and ops.Stem, and one end-to-end pair (the whole pyramid
against its propagated bound in both modes, then estimate_matches_device in the full fast configuration)."""
import copy

import numpy as np
import pytest
import torch

import backbone_mode_reference as bm
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from patch2pix_amd import ops
    return ops


_CACHE = {}


def _run(ops, dev, case, modes=(), tile=None, first_image_only=False):
    """One launch of a case through ops.ConvBN (cached per (case, modes, tile)) -> (y NCHW on the host, max |y| per image as the
    kernel reports it)."""
    key = (case, modes, tile, first_image_only)
    if key in _CACHE:
        return _CACHE[key]
    wt, bn, x, sk = bm.case_inputs(case)
    _, _, _, stride, _, relu = bm.LAYERS[case[0]]
    if first_image_only:
        x, sk = x[:1], None if sk is None else sk[:1]
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("P2P_BACKBONE_MODE", raising=False)
        mp.setattr(ops, "FORCED_CONV_TILE", tile)
        cv = ops.ConvBN(wt, *bn, stride, dev)
        assert cv.mode == "fp16x2"
        for m in modes:
            cv.set_mode(m)
            assert cv.mode == m
        xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
        res = None if sk is None else sk.permute(0, 2, 3, 1).contiguous().to(dev)
        ymax = torch.zeros(x.shape[0], device=dev, dtype=torch.int32)
        y = cv.forward(xn, ops.absmax_batch(xn), residual=res, relu=relu, ymax=ymax)
        torch.cuda.synchronize()
    finally:
        mp.undo()
    _CACHE[key] = y.permute(0, 3, 1, 2).contiguous().cpu(), ymax.cpu().view(torch.float32)
    return _CACHE[key]


def test_mode_is_selectable(ops, dev, monkeypatch):
    wt, bn, _, _ = bm.case_inputs(("l1_3x3", (8, 16)))
    monkeypatch.delenv("P2P_BACKBONE_MODE", raising=False)
    cv = ops.ConvBN(wt, *bn, 1, dev)
    assert cv.mode == "fp16x2"
    cv.set_mode("fp16")
    assert cv.mode == "fp16"
    with pytest.raises(ValueError, match="fp16"):
        cv.set_mode("fp8")
    assert cv.mode == "fp16"
    monkeypatch.setenv("P2P_BACKBONE_MODE", "fp16")          # new handles start in the environment's mode
    swt, sbn, _ = bm.stem_inputs()
    assert ops.ConvBN(wt, *bn, 1, dev).mode == "fp16" and ops.Stem(swt, *sbn, dev).mode == "fp16"
    monkeypatch.setenv("P2P_BACKBONE_MODE", "half")
    with pytest.raises(ValueError):
        ops.ConvBN(wt, *bn, 1, dev)


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_error_bounds_in_both_modes(case, ops, dev, capsys):
    """|out - fp64| <= bound element-wise in mode 'fp16'; (a) the default mode inside its own bound; (b) the outputs differ."""
    fast, _ = _run(ops, dev, case, ("fp16",))
    default, _ = _run(ops, dev, case)
    with capsys.disabled():
        print()
        bm.check_layer(fast, case, "fp16", "MI355X ")
        bm.check_layer(default, case, "fp16x2", "MI355X ")
    assert not torch.equal(fast, default), "mode 'fp16' gave the default mode's bits"


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_tile_independence_inside_the_mode(case, ops, dev):
    fast, fmax = _run(ops, dev, case, ("fp16",))
    for tile in bm.tiles_of(bm.LAYERS[case[0]][1]):
        got, gmax = _run(ops, dev, case, ("fp16",), tile)
        assert torch.equal(got, fast) and torch.equal(gmax, fmax), f"tile {tile}"
    assert torch.equal(fmax, fast.abs().amax(dim=(1, 2, 3)))


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_batch_independence_inside_the_mode(case, ops, dev):
    fast, fmax = _run(ops, dev, case, ("fp16",))
    one, omax = _run(ops, dev, case, ("fp16",), None, True)
    assert torch.equal(one[0], fast[0]) and torch.equal(omax[0], fmax[0])


@pytest.mark.parametrize("case", bm.CASES, ids=bm.case_id)
def test_default_mode_untouched(case, ops, dev):
    """A handle whose mode was never set, one set to 'fp16x2' and one switched 'fp16' -> 'fp16x2': the same bits."""
    never, nmax = _run(ops, dev, case)
    for modes in (("fp16x2",), ("fp16", "fp16x2")):
        got, gmax = _run(ops, dev, case, modes)
        assert torch.equal(got, never) and torch.equal(gmax, nmax), modes


def test_stem_bounds_and_round_trip(ops, dev, monkeypatch, capsys):
    monkeypatch.delenv("P2P_BACKBONE_MODE", raising=False)
    wt, bn, image = bm.stem_inputs()
    st = ops.Stem(wt, *bn, dev)
    never = st.forward(image.to(dev)).cpu()
    st.set_mode("fp16")
    fast = st.forward(image.to(dev)).cpu()
    one = st.forward(image[:1].contiguous().to(dev)).cpu()
    st.set_mode("fp16x2")
    back = st.forward(image.to(dev)).cpu()
    with capsys.disabled():
        print()
        bm.check_stem(fast, "fp16", "MI355X ")
        bm.check_stem(never, "fp16x2", "MI355X ")
    assert not torch.equal(fast, never) and torch.equal(back, never) and torch.equal(one[0], fast[0])


def _images(seeds, h, w):
    ims = [synthetic.make_image_pair(s, h, w)[0] for s in seeds]
    x = torch.stack([torch.from_numpy(a).permute(2, 0, 1).float() / 255.0 for a in ims])
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (x - mean) / std


def test_pyramid_and_matches_end_to_end(dev, tmp_path, monkeypatch, capsys):
    """A 64 x 96 pair (layer3 map 8 x 12): every pyramid level within the propagated bound of its mode against the fp64 walk of
    the same module; then estimate_matches_device with the backbone and both regressors in 'fp16' returns a well-formed triple.
    The share of its coarse rows that the default configuration also returns is printed, not asserted (near-ties of the
    correlation volume may fall the other way in this mode)."""
    from PIL import Image
    from patch2pix_amd.utils.eval import model_helper
    monkeypatch.delenv("P2P_BACKBONE_MODE", raising=False)
    monkeypatch.setenv("P2P_BACKBONE", "hip")
    net = model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)
    host_extract = copy.deepcopy(net.extract).cpu().float().eval()
    x = _images([31, 32], 64, 96)
    lines = []
    _, mid, fine = net._weights()
    try:
        for mode in ("fp16x2", "fp16"):
            net.extract.set_mode(mode)
            assert net.extract.mode == mode
            with torch.no_grad():
                got = [t.cpu() for t in net.extract.pyramid(x.to(dev))]
            levels, bounds = bm.pyramid_yardstick(host_extract, x, mode)
            assert len(got) == 5
            for lv in range(5):
                assert got[lv].shape == levels[lv].shape and torch.isfinite(got[lv]).all()
                err = (got[lv].double() - levels[lv]).abs()
                ratio = (err / bounds[lv].clamp_min(1e-300)).max().item()
                rel = (err.amax(dim=(1, 2, 3)) / levels[lv].abs().amax(dim=(1, 2, 3))).max().item()
                lines.append(f"pyramid 64x96 mode {mode} level {lv}: max |err| {err.max().item():.3e} ({rel:.2e} of the largest "
                             f"value), max err / bound {ratio:.4f}")
                assert ratio <= 1.0, lines[-1]
        im1, im2 = synthetic.make_image_pair(33, 64, 96)
        Image.fromarray(im1).save(tmp_path / "1.png")
        Image.fromarray(im2).save(tmp_path / "2.png")
        paths = (str(tmp_path / "1.png"), str(tmp_path / "2.png"))
        net.extract.set_mode("fp16x2")
        base = model_helper.estimate_matches_device(net, *paths, ksize=2, io_thres=0.25)
        net.extract.set_mode("fp16")
        mid.set_mode("fp16")
        fine.set_mode("fp16")
        m, s, c = model_helper.estimate_matches_device(net, *paths, ksize=2, io_thres=0.25)
    finally:
        net.extract.set_mode("fp16x2")
        mid.set_mode("fp16x2w")
        fine.set_mode("fp16x2w")
    assert m.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64
    assert m.ndim == 2 and m.shape[1] == 4 and c.shape == m.shape and s.shape == (m.shape[0],) and m.shape[0] > 0
    assert np.isfinite(m).all() and np.isfinite(s).all() and np.isfinite(c).all() and (s >= 0).all() and (s <= 1).all()
    assert (c >= 0).all() and (c[:, [0, 2]] <= 96).all() and (c[:, [1, 3]] <= 64).all()
    known = {tuple(r) for r in base[2].tolist()}
    share = sum(tuple(r) in known for r in c.tolist()) / c.shape[0]
    lines.append(f"full fast configuration, 64x96 pair: {c.shape[0]} rows ({base[2].shape[0]} in the default configuration), "
                 f"share of coarse rows the default configuration also returns {share:.3f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
