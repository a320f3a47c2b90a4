"""Coarse mode 'fp16' (P2P_COARSE_FP16) on the MI355X through the real library: the stage bounds, the index assertions and the
equalities of tests/test_coarse_mode_emulated.py on every case of tests/coarse_mode_reference.py (ksize 4 included), the
setter's errors, and one end-to-end 128 x 160 pair through Patch2Pix and GraphedMatcher."""
import numpy as np
import pytest
import torch

import coarse_mode_reference as cm
import golden_util as gu
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from patch2pix_amd import _lib
    assert "p2p_ncn_set_mode" in _lib.EXPORTS
    return _lib.lib


def _sd():
    return gu.state_dict(0)


_CACHE = {}


def _run(lib, dev, name, modes=(), tile=None, pair=None, ws_pairs=None):
    """One coarse stage of a case through the C ABI on a fresh handle (cached per variant) -> run_coarse's dict + rows, scores."""
    key = (name, modes, tile, pair, ws_pairs)
    if key in _CACHE:
        return _CACHE[key]
    fa, fb = cm.case_inputs(name)
    if pair is not None:
        fa, fb = fa[pair:pair + 1], fb[pair:pair + 1]
    with torch.cuda.device(dev):
        ncn = cm.ncn_create(lib, _sd())
        try:
            assert lib.p2p_ncn_get_mode(ncn) == 0
            for m in modes:
                cm.set_mode(lib, ncn, m)
            if tile:
                assert lib.p2p_ncn_set_tile(ncn, *tile) == 0
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = cm.run_coarse(lib, ncn, fa.to(dev), fb.to(dev), cm.CASES[name][3], ws_pairs=ws_pairs, stream=stream)
            out["rows"], out["scores"] = cm.run_matches(lib, out["corr"], out["delta"], cm.CASES[name][3], stream=stream)
        finally:
            lib.p2p_ncn_destroy(ncn)
    _CACHE[key] = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
    return _CACHE[key]


def test_setter_errors(lib, dev):
    from patch2pix_amd import ops
    sd = {k[len("ncn."):]: v for k, v in _sd().items() if k.startswith("ncn.")}
    w = ops.NcnWeights.from_state_dict(sd, dev)
    assert w.mode == "fp16x2"
    w.set_mode("fp16")
    assert w.mode == "fp16"
    for bad in ("fp32", "FP16", "", None, 1):
        with pytest.raises(ValueError):
            w.set_mode(bad)
    assert w.mode == "fp16"
    assert lib.p2p_ncn_set_mode(w.handle, 5) == -1 and lib.p2p_ncn_get_mode(w.handle) == 1
    assert lib.p2p_ncn_set_mode(None, 1) == -1 and lib.p2p_ncn_get_mode(None) == -1
    g = ops.NcnWeights.from_state_dict(sd, dev, generic=True)
    with pytest.raises(NotImplementedError):
        g.set_mode("fp16")
    assert lib.p2p_ncn_set_mode(g.handle, 1) == -3 and lib.p2p_ncn_get_mode(g.handle) == 0


@pytest.mark.parametrize("name", cm.ALL_CASES)
def test_stage_bounds_and_rows_in_both_modes(name, lib, dev, capsys):
    """Every stage output within its bound in both modes, the outputs differ, every decidable row names the fp64 winner and
    the modes differ only on rows that are undecidable under the 'fp16' bound."""
    share = cm.assert_decidable_share(name, _sd())
    fast, default = _run(lib, dev, name, ("fp16",)), _run(lib, dev, name)
    rf = cm.check_stages(fast, name, _sd(), "fp16", "MI355X ")
    rd = cm.check_stages(default, name, _sd(), "fp16x2", "MI355X ")
    assert not torch.equal(fast["corr"], default["corr"]) and not torch.equal(fast["x"], default["x"])
    bad_f, dec_f, tot = cm.check_rows(fast["rows"], name, _sd(), "fp16")
    bad_d, dec_d, _ = cm.check_rows(default["rows"], name, _sd(), "fp16x2")
    dec = torch.cat([y.decidable()[1] for y in cm.yardsticks(name, _sd(), "fp16")]).view(fast["rows"].shape[0], -1)
    differ = (fast["rows"] != default["rows"]).any(dim=-1)
    assert not bool((differ & dec).any()), "the modes differ on a row that is decidable under the fp16 bound"
    with capsys.disabled():
        fmt = lambda r: ", ".join(f"{k} {v:.4f}" for k, v in r.items())
        print(f"\nMI355X {name}: decidable share {share:.3f}; measured / bound fp16: {fmt(rf)}; fp16x2: {fmt(rd)}; rows differing "
              f"from fp64: fp16 {bad_f}, fp16x2 {bad_d} of {tot}; rows differing between the modes {int(differ.sum())}")


@pytest.mark.parametrize("name", cm.ALL_CASES)
def test_default_mode_untouched(name, lib, dev):
    """A handle that never saw the setter and one switched to 'fp16' and back give identical bits."""
    never, back = _run(lib, dev, name), _run(lib, dev, name, ("fp16", "fp16x2"))
    for key in ("corr", "delta", "x", "y", "rows", "scores"):
        assert (never[key] is None and back[key] is None) or torch.equal(never[key], back[key]), key


def test_tile_batch_and_workspace_independence_inside_the_mode(lib, dev):
    base = _run(lib, dev, "c32_12x16_k1_tiles", ("fp16",))
    for tile in ((2, 3, 2), (4, 6, 6), (0, 2, 5), (3, 4, 3), (12, 10, 8), (1, 5, 8)):
        got = _run(lib, dev, "c32_12x16_k1_tiles", ("fp16",), tile)
        assert torch.equal(got["corr"], base["corr"]) and torch.equal(got["y"], base["y"]), f"tile {tile} changes the volume"
    name = "c32_8x8_k2_batch3"
    batch, small = _run(lib, dev, name, ("fp16",)), _run(lib, dev, name, ("fp16",), None, None, 1)
    assert torch.equal(small["corr"], batch["corr"]) and torch.equal(small["delta"], batch["delta"])
    for z in range(3):
        one = _run(lib, dev, name, ("fp16",), None, z)
        assert torch.equal(one["corr"][0], batch["corr"][z]) and torch.equal(one["delta"][0], batch["delta"][z]), f"pair {z}"
        assert torch.equal(one["x"][0], batch["x"][z]) and torch.equal(one["y"][0], batch["y"][z])


def test_consensus_entry_point_equals_the_stage_leg(lib, dev):
    name = "c32_12x16_k1_tiles"
    for modes in ((), ("fp16",)):
        stage = _run(lib, dev, name, modes)
        with torch.cuda.device(dev):
            ncn = cm.ncn_create(lib, _sd())
            try:
                for m in modes:
                    cm.set_mode(lib, ncn, m)
                y = cm.run_consensus(lib, ncn, stage["x"].to(dev), stream=torch.cuda.current_stream(dev).cuda_stream).cpu()
            finally:
                lib.p2p_ncn_destroy(ncn)
        assert torch.equal(y, stage["y"]), modes


def _norm_images(seeds, h, w, dev):
    ims = [synthetic.make_image_pair(s, h, w) for s in seeds]
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    to_t = lambda a: ((torch.from_numpy(np.stack(a)).permute(0, 3, 1, 2).float() / 255.0 - mean) / std).to(dev)
    return to_t([p[0] for p in ims]), to_t([p[1] for p in ims])


def test_end_to_end_pair(dev, tmp_path, monkeypatch, capsys):
    """A 128 x 160 seeded pair: Patch2Pix.set_coarse_mode('fp16') survives load_state_dict; forward, predict_coarse, predict_fine
    and estimate_matches_device run, also with all three stages in 'fp16'; GraphedMatcher replays the mode's bits; the coarse
    rows differ from the default mode's only where the row is undecidable under the 'fp16' bound."""
    from PIL import Image
    from patch2pix_amd.utils.eval import model_helper
    from patch2pix_amd.utils.eval.graphed import GraphedMatcher
    for var in ("P2P_COARSE_MODE", "P2P_BACKBONE_MODE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("P2P_BACKBONE", "hip")
    net = model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)
    assert net.coarse_mode == "fp16x2" and net._weights()[0].mode == "fp16x2"
    with pytest.raises(ValueError):
        net.set_coarse_mode("half")
    im1, im2 = _norm_images([41], 128, 160, dev)
    with torch.no_grad():
        f1, f2 = net._pyramids(im1, im2)
        corr_d, delta_d = net.forward_coarse_match(f1[-1], f2[-1], ksize=2)
        rows_d, _ = net.cal_coarse_matches(corr_d, delta_d, ksize=2, upsample=net.upsample)
        net.set_coarse_mode("fp16")
        assert net.coarse_mode == "fp16" and net._weights()[0].mode == "fp16"
        net.load_state_dict(net.state_dict())                       # re-pack: the model keeps the choice
        assert net._packed is None and net._weights()[0].mode == "fp16" and net.coarse_mode == "fp16"
        corr_f, delta_f = net.forward_coarse_match(f1[-1], f2[-1], ksize=2)
        rows_f, _ = net.cal_coarse_matches(corr_f, delta_f, ksize=2, upsample=net.upsample)
        torch.cuda.synchronize()
        assert not torch.equal(corr_f, corr_d)
        # differing rows are undecidable under the fp16 bound of THIS pair's features
        yd = cm.Yardstick(f1[-1][0].cpu(), f2[-1][0].cpu(), 2, gu.state_dict(0), "fp16")
        _, dec = yd.decidable()
        differ = (rows_f[0] != rows_d[0]).any(dim=-1).cpu()
        assert not bool((differ & dec).any()), f"{int((differ & dec).sum())} decidable coarse rows moved in mode fp16"
        err = (corr_f[0, 0].cpu().double() - yd.z).abs()
        assert bool((err <= yd.e_z).all())
        # every public path runs in the mode
        c4, d4 = net.forward(im1, im2, ksize=2)
        assert torch.equal(c4, corr_f) and torch.equal(d4.packed, delta_f.packed)
        cm_, cs_ = net.predict_coarse(im1, im2, ksize=2)
        fine, scores, coarse = net.predict_fine(im1, im2, ksize=2)
        assert len(fine) == 1 and fine[0].shape[1] == 4 and torch.isfinite(fine[0]).all() and fine[0].shape[0] > 0
        g = GraphedMatcher(net, 128, 160)
        gf, gs, gc = g(im1, im2)
        assert torch.equal(gf[0], fine[0]) and torch.equal(gs[0], scores[0]) and torch.equal(gc[0], coarse[0])
        # all three stages in fp16 together, from image files
        a, b = synthetic.make_image_pair(41, 128, 160)
        Image.fromarray(a).save(tmp_path / "1.png")
        Image.fromarray(b).save(tmp_path / "2.png")
        _, mid, fine_w = net._weights()
        try:
            net.extract.set_mode("fp16")
            mid.set_mode("fp16")
            fine_w.set_mode("fp16")
            m, s, c = model_helper.estimate_matches_device(net, str(tmp_path / "1.png"), str(tmp_path / "2.png"), ksize=2, io_thres=0.25)
        finally:
            net.extract.set_mode("fp16x2")
            mid.set_mode("fp16x2w")
            fine_w.set_mode("fp16x2w")
        assert m.ndim == 2 and m.shape[1] == 4 and m.shape[0] > 0 and np.isfinite(m).all() and np.isfinite(s).all()
        net.set_coarse_mode("fp16x2")
        back, _ = net.forward_coarse_match(f1[-1], f2[-1], ksize=2)
        assert torch.equal(back, corr_d)
    with capsys.disabled():
        print(f"\nend to end 128x160: {int(differ.sum())} of {differ.numel()} coarse rows differ between the modes, "
              f"{int(dec.sum())} rows decidable under the fp16 bound; all three stages in fp16: {m.shape[0]} matches")
