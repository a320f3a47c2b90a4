"""The pair score on the MI355X: the checks of tests/test_score_emulated.py through the real library (with case T, the pooled
volume of a 240x320 pair), Patch2Pix.cal_coarse_score on the volume net.forward returns, and predict_score / estimate_score
end to end, with a full and with an NC-only model.
Needs an MI355X:  pytest -m gpu"""
import os

import pytest
import torch

import golden_util as gu
import score_reference as sr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu

CASE_NORMS = [(c, n) for c in sr.CASES for n in sr.NORMS]
IDS = [f"{c}-{sr.norm_tag(n)}" for c, n in CASE_NORMS]
GOLDEN_NORMS = [(c, n) for c in sr.HOST_CASES for n in sr.NORMS]
GOLDEN_IDS = [f"{c}-{sr.norm_tag(n)}" for c, n in GOLDEN_NORMS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from patch2pix_amd import _lib
    return sr.bind(_lib.lib)


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


@pytest.fixture(scope="module")
def pair_240x320(dev):
    im1, im2 = synthetic.make_image_pair(11, 240, 320)
    to = lambda im: torch.from_numpy(im).permute(2, 0, 1).float().div(255)[None].to(dev)
    return to(im1), to(im2)


@pytest.mark.parametrize("case,normalize", CASE_NORMS, ids=IDS)
def test_scores(case, normalize, lib, dev):
    sr.check_case(lib, case, normalize, dev)


@pytest.mark.parametrize("case,normalize", GOLDEN_NORMS, ids=GOLDEN_IDS)
def test_scores_against_reference_golden(case, normalize, lib, dev):
    sr.check_against_golden(lib, case, normalize, dev)


def test_ops_return_cells(dev):
    """ops.coarse_score_batch: [B] alone, ([B], [B, nA+nB]) with return_cells, equal to the raw entry point bit for bit."""
    from patch2pix_amd import _lib, ops
    corr = sr.inputs("W", "l1").to(dev)
    pair, cells = ops.coarse_score_batch(corr, "l1", return_cells=True)
    alone = ops.coarse_score_batch(corr, "l1")
    rc, rp = sr.run_score(sr.bind(_lib.lib), corr, "l1")
    assert pair.shape == (3,) and cells.shape == (3, 70 + 65) and pair.dtype == cells.dtype == torch.float32 and pair.is_cuda
    assert torch.equal(pair.cpu(), rp) and torch.equal(cells.cpu(), rc) and torch.equal(alone, pair)


@pytest.mark.parametrize("normalize", sr.NORMS, ids=[sr.norm_tag(n) for n in sr.NORMS])
def test_cal_coarse_score_on_the_model_volume(normalize, net, pair_240x320, dev):
    """cal_coarse_score on the corr4d net.forward returns for a 240x320 pair (15x20x15x20 cells at ksize 2): a 0-dim device
    tensor equal to the restatement on that volume, and to the mean of the scores cal_coarse_matches gives (softmax; raw
    scores through do_softmax=False)."""
    corr4d, delta4d = net.forward(*pair_240x320, ksize=2)
    assert corr4d.shape == (1, 1, 15, 20, 15, 20)
    score = net.cal_coarse_score(corr4d, normalize=normalize)
    assert score.dim() == 0 and score.is_cuda and score.dtype == torch.float32
    # the consensus volume is non-negative (MutualMatching of ReLU outputs): l1 scores lie in [0, 1]
    assert bool((corr4d >= 0).all())
    _, _, want = sr.restate(corr4d[:, 0], normalize)
    case = "T"          # the bars of a non-negative volume
    sr.assert_within(f"cal_coarse_score {sr.norm_tag(normalize)} against the restatement", score.cpu(), want, case, normalize)
    if normalize != "l1":
        _, s = net.cal_coarse_matches(corr4d, delta4d, ksize=2, do_softmax=normalize == "softmax", upsample=net.upsample)
        sr.assert_within(f"cal_coarse_score {sr.norm_tag(normalize)} against cal_coarse_matches", score.cpu(), s.double().mean().cpu(),
                         case, normalize)
    with pytest.raises(ValueError, match="normalize"):
        net.cal_coarse_score(corr4d, normalize="l2")


def test_predict_score_batch_equals_single_pairs(net, pair_240x320, dev):
    """predict_score of a batch of two pairs (the pair and the pair swapped) == the two single-pair calls, bit for bit; and
    == cal_coarse_score of each pair's own volume."""
    t1, t2 = pair_240x320
    a, b = torch.cat([t1, t2]), torch.cat([t2, t1])
    for normalize in sr.NORMS:
        both = net.predict_score(a, b, ksize=2, normalize=normalize)
        assert both.shape == (2,) and both.dtype == torch.float32 and both.is_cuda
        one = [net.predict_score(a[i:i + 1], b[i:i + 1], ksize=2, normalize=normalize) for i in range(2)]
        assert torch.equal(both.view(torch.int32), torch.cat(one).view(torch.int32)), normalize
        corr4d, _ = net.forward(a[:1], b[:1], ksize=2)
        assert torch.equal(net.cal_coarse_score(corr4d, normalize).view(torch.int32), both[0].view(torch.int32))
    feats1, feats2 = net._pyramids(a, b)
    assert torch.equal(net.score_from_feats(feats1, feats2, ksize=2, normalize="l1"), net.predict_score(a, b, normalize="l1"))
    with pytest.raises(ValueError, match="normalize"):
        net.predict_score(a, b, normalize="max")


def _photo(pair, which):
    return os.path.join(gu.GOLDEN, "images", pair, f"{which}.jpg")


def test_estimate_score_on_a_photograph_pair(net, dev):
    """estimate_score on one of the reference's example pairs (loaded at imsize 256) == predict_score on the tensors
    estimate_matches loads, as a Python float in [0, 1]."""
    from patch2pix_amd.utils.eval import model_helper
    im1, im2 = _photo("pair_1", 1), _photo("pair_1", 2)
    t1, t2, _ = model_helper._load_pair(net, im1, im2, 2, 256)
    for normalize in ("softmax", "l1"):
        got = model_helper.estimate_score(net, im1, im2, ksize=2, normalize=normalize, imsize=256)
        want = net.predict_score(t1, t2, ksize=2, normalize=normalize)
        assert isinstance(got, float) and 0.0 < got <= 1.0
        assert got == float(want[0]), normalize
    with pytest.raises(ValueError, match="normalize"):
        model_helper.estimate_score(net, im1, im2, normalize="none")


def test_nc_only_model_scores(pair_240x320, net, dev):
    """load_model(method='nc'): no regressors, the same calls; an NC-only model with the full model's backbone and consensus
    weights gives the full model's scores bit for bit."""
    from patch2pix_amd.utils.eval import model_helper
    nc_sd = {k: v for k, v in gu.state_dict(0).items() if k.startswith(("extract.", "ncn."))}
    nc = model_helper.load_model({"state_dict": nc_sd}, method="nc", lprint=lambda *a: None)
    assert nc.regress_mid is None
    t1, t2 = pair_240x320
    for normalize in sr.NORMS:
        s = nc.predict_score(t1, t2, ksize=2, normalize=normalize)
        assert s.shape == (1,) and bool(torch.isfinite(s).all())
        assert torch.equal(s.view(torch.int32), net.predict_score(t1, t2, ksize=2, normalize=normalize).view(torch.int32))
    corr4d, _ = nc.forward(t1, t2, ksize=2)
    assert torch.equal(nc.cal_coarse_score(corr4d).view(torch.int32), nc.predict_score(t1, t2)[0].view(torch.int32))
