"""The top-k match extraction on the MI355X: the parity checks of tests/test_topk_emulated.py through the real library,
cal_coarse_matches(do_softmax=False), and predict_coarse_topk / predict_fine_topk end to end on a small synthetic pair.
Needs an MI355X:  pytest -m gpu"""
import pytest
import torch

import topk_reference as tr
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from patch2pix_amd import _lib
    return tr.bind(_lib.lib)


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_topk_against_restatement(case, lib, dev):
    tr.check_against_restatement(lib, case, dev)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_one_candidate_against_restatement(case, lib, dev):
    tr.check_one_candidate_against_restatement(lib, case, dev)


@pytest.mark.parametrize("case", tr.GOLDEN_CASES)
def test_topk_against_reference_golden(case, lib, dev):
    tr.check_against_golden(lib, case, dev)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_topk_1_is_the_one_candidate_kernels(case, lib, dev):
    tr.check_top1_identity(lib, case, dev)


def test_cal_coarse_matches_without_softmax(net, dev):
    """do_softmax=False of the model class on case W: the restatement with one candidate, raw scores bit for bit; sort=True
    orders them."""
    c = tr.CASES["W"]
    corr, delta = tr.inputs("W", False)
    from patch2pix_amd.networks.patch2pix import Delta4d
    m, s = net.cal_coarse_matches(corr.to(dev).unsqueeze(1), Delta4d(delta.to(dev), c["ksize"]), ksize=c["ksize"],
                                  do_softmax=False, upsample=c["upsample"], center=c["center"])
    rm, rs = tr.restate(corr, delta, c["ksize"], c["upsample"], c["center"], 1, False)
    assert torch.equal(m.cpu(), rm)
    assert torch.equal(s.cpu().view(torch.int32), rs.view(torch.int32))
    _, ss = net.cal_coarse_matches(corr.to(dev).unsqueeze(1), Delta4d(delta.to(dev), c["ksize"]), ksize=c["ksize"],
                                   do_softmax=False, upsample=c["upsample"], center=c["center"], sort=True)
    assert (ss[:, :-1] >= ss[:, 1:]).all() and torch.equal(ss.cpu().sort(dim=1)[0], rs.sort(dim=1)[0])


def _image_pair(dev):
    im1, im2 = synthetic.make_image_pair(9, 96, 128)
    to = lambda im: torch.from_numpy(im).permute(2, 0, 1).float().div(255)[None].to(dev)
    return to(im1), to(im2)


def test_predict_topk_end_to_end(net, dev):
    """96x128 pair, topk 2, ksize 2 (6x8 cells per image): the coarse list is the restatement of the model's own volume and
    delta (same input bits: no near-tie to adjudicate), 2 * (nA + nB) rows before filtering; the fine stage is _fine_chain
    on the filtered list, bit for bit."""
    from patch2pix_amd.networks.utils import filter_coarse
    topk, ksize = 2, 2
    t1, t2 = _image_pair(dev)
    corr4d, delta4d = net.forward(t1, t2, ksize=ksize)
    assert corr4d.shape == (1, 1, 6, 8, 6, 8)
    m, s = net.cal_coarse_matches_topk(corr4d, delta4d, topk, ksize=ksize, upsample=net.upsample, center=True)
    assert m.shape == (1, topk * (48 + 48), 4) and s.shape == (1, topk * (48 + 48))
    rm, rs = tr.restate(corr4d[:, 0], delta4d.packed, ksize, net.upsample, True, topk, True)
    assert torch.equal(m.cpu(), rm)
    assert (s.cpu() - rs).abs().max() <= tr.SCORE_TOL
    # every candidate of rank 1 scores no more than its rank 0
    nB = 48
    assert (s[0, nB:2 * nB] <= s[0, :nB]).all() and (s[0, 2 * nB + 1::2] <= s[0, 2 * nB::2]).all()

    coarse, cscores = net.predict_coarse_topk(t1, t2, topk, ksize=ksize)
    want, wscores = filter_coarse(rm.to(dev), rs.to(dev), 0.0, False)
    assert len(coarse) == 1 and torch.equal(coarse[0].cpu(), want[0].cpu())
    assert (cscores[0].cpu() - wscores[0].cpu()).abs().max() <= tr.SCORE_TOL
    one, _ = net.predict_coarse(t1, t2, ksize=ksize)
    rows = lambda t: set(map(tuple, t.cpu().tolist()))
    assert rows(one[0]) <= rows(coarse[0]), "the one-candidate proposals are the rank 0 of the top-k list"

    fine, fscores, mid, mscores, used = net.predict_fine_topk(t1, t2, topk, ksize=ksize, return_all=True)
    feats1, feats2 = net._pyramids(t1, t2)
    filtered, _ = filter_coarse(m, s, 0.0, True)
    filtered = net.shift_to_anchors(filtered)
    assert torch.equal(used[0], filtered[0])
    rf, rfs, rmid, rms = net._fine_chain(feats1, feats2, filtered)
    assert torch.equal(fine[0], rf[0]) and torch.equal(fscores[0], rfs[0])
    assert torch.equal(mid[0], rmid[0]) and torch.equal(mscores[0], rms[0])
    assert fine[0].shape == (filtered[0].shape[0], 4)
    short = net.predict_fine_topk(t1, t2, topk, ksize=ksize)
    assert len(short) == 3 and torch.equal(short[0][0], fine[0])
