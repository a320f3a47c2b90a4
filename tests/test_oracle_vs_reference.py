"""Pin the CPU oracle (oracle/p2p_oracle.py) against the unmodified reference, function by
function, on seeded inputs.  The reference's answers on exactly these inputs are stored in
tests/golden/oracle_pins.npz (oracle/make_golden.py --pins), so the tests run anywhere."""
import numpy as np
import pytest
import torch

from golden_util import checksum, load
from oracle import p2p_oracle as orc
from oracle.make_golden import PIN_SD_SEED, pin_feats, pin_fine_inputs
from patch2pix_amd.utils import synthetic


@pytest.fixture(scope="module")
def pins():
    return load("oracle_pins")


@pytest.fixture(scope="module")
def sd(pins):
    assert int(pins["sd_seed"]) == PIN_SD_SEED
    return synthetic.make_state_dict(PIN_SD_SEED)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same_input(got, want):
    assert abs(got - float(want)) <= 1e-6 * float(want), "seeded inputs drifted from the ones the fixture was made with"


def test_l2norm_and_correlation(pins):
    fa, fb = pin_feats(0, 6, 8), pin_feats(1, 4, 10)
    _same_input(checksum([fa, fb]), pins["corr_input_checksum"])
    ref = _t(pins["corr"])
    got = orc.correlation(orc.l2_normalize(fa, 0), orc.l2_normalize(fb, 0))
    assert torch.allclose(got, ref, atol=1e-6)


def test_maxpool4d_with_ties(pins):
    g = torch.Generator().manual_seed(5)
    corr = torch.randint(0, 3, (8, 12, 6, 10), generator=g).float()     # many exact ties
    assert torch.equal(corr, _t(pins["maxpool_input"]))
    pooled, delta = orc.maxpool4d(corr, 2)
    assert torch.equal(pooled, _t(pins["maxpool_pooled"]))
    assert len(delta) == pins["maxpool_delta"].shape[0]
    for d, r in zip(delta, pins["maxpool_delta"]):
        assert torch.equal(d, _t(r))


def test_mutual_matching(pins):
    x = torch.rand(5, 6, 7, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(x, _t(pins["mutual_input"]))
    assert torch.equal(orc.mutual_matching(x), _t(pins["mutual"]))


def test_conv4d_and_consensus(pins, sd):
    ncn, _, _ = orc.split_params(sd)
    x = torch.rand(6, 8, 5, 7, generator=torch.Generator().manual_seed(9))
    assert torch.equal(x, _t(pins["conv4d_input"]))
    ref1, ref = _t(pins["conv4d_layer1"]), _t(pins["consensus"])
    got1 = orc.conv4d(x[None], ncn["w1"], ncn["b1"])
    assert torch.allclose(got1, ref1, atol=2e-6)
    assert torch.allclose(orc.neigh_consensus(x, ncn), ref, atol=5e-6)


def test_coarse_forward_and_matches(pins, sd):
    ncn, _, _ = orc.split_params(sd)
    fa, fb = pin_feats(10, 8, 12), pin_feats(11, 8, 12)
    _same_input(checksum([fa, fb]), pins["coarse_input_checksum"])
    rm, rs = _t(pins["coarse_matches"]), _t(pins["coarse_scores"])
    corr, delta = orc.coarse_forward(fa, fb, 2, ncn)
    assert torch.allclose(corr, _t(pins["coarse_corr"]), rtol=1e-4, atol=1e-7)
    assert len(delta) == pins["coarse_delta"].shape[0]
    for d, r in zip(delta, pins["coarse_delta"]):
        assert torch.equal(d, _t(r))
    m, s = orc.cal_coarse_matches(corr, delta, 2, 8)
    assert torch.equal(m, rm)
    assert torch.allclose(s, rs, rtol=1e-5)
    # filter_coarse, both modes, and the ptmax shuffle with the same numpy seed
    for mutual in (True, False):
        rf, rfs = _t(pins[f"filter_mutual{int(mutual)}"]), _t(pins[f"filter_mutual{int(mutual)}_scores"])
        f, fs = orc.filter_coarse(m, s, 0.0, mutual)
        assert torch.equal(f, rf) and torch.allclose(fs, rfs, rtol=1e-5)
    rf = _t(pins["filter_ptmax50"])
    f, _ = orc.filter_coarse(m, s, 0.0, True, ptmax=50, rng=np.random.RandomState(4))
    assert torch.equal(f, rf) and f.shape[0] == 50


def test_shift_to_anchors(pins):
    m = torch.randint(0, 100, (7, 4), generator=torch.Generator().manual_seed(6))
    assert torch.equal(m, _t(pins["anchors_input"]))
    assert torch.equal(orc.shift_to_anchors(m, 8, 8), _t(pins["anchors"]))


@pytest.mark.parametrize("as_float", [False, True])
def test_fine_level(pins, sd, as_float):
    _, mid_p, fine_p = orc.split_params(sd)
    p1, p2, m = pin_fine_inputs(as_float)
    _same_input(checksum(p1 + p2 + [m]), pins[f"fine{int(as_float)}_input_checksum"])
    rm, rp = _t(pins[f"fine{int(as_float)}_matches"]), _t(pins[f"fine{int(as_float)}_scores"])
    got_m, got_p, raw = orc.fine_level(p1[:4], p2[:4], m, mid_p)
    assert torch.allclose(got_m, rm, atol=2e-4)
    assert torch.allclose(got_p, rp, atol=1e-5)
    # the offsets must be in the sensitive range, otherwise this test proves nothing
    off = (got_m - m.float()).abs()
    assert off.max() > 0.5 and (raw[:, :4] > 0).any()


def test_predict_fine_end_to_end(pins, sd):
    H, W = 64, 96
    p1, p2 = synthetic.make_correlated_pyramids(31, H, W)
    _same_input(checksum(p1 + p2), pins["e2e_input_checksum"])
    out = orc.predict_fine(p1, p2, sd)
    assert torch.equal(out["coarse"], _t(pins["e2e_coarse"]))
    assert out["coarse"].shape[0] >= 8
    assert torch.allclose(out["mid"], _t(pins["e2e_mid"]), atol=2e-4)
    assert torch.allclose(out["fine"], _t(pins["e2e_fine"]), atol=1e-3)
    assert torch.allclose(out["fine_scores"], _t(pins["e2e_fine_scores"]), atol=1e-5)
