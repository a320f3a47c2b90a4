"""Regressor parity over dynamic range on the MI355X:  pytest -m gpu

The stress families of tests/stress_inputs.py (pyramids with a wide dynamic range inside one patch; checkpoints with
negative BatchNorm weights, spread variances, dead channels, per-channel octaves and exact re-parametrisations) at
96 x 128 with 64 proposals per case through ops.regress (mid + fine), in all three arithmetic modes, against
orc.fine_level evaluated in fp64 -- the project's bars, unchanged: coordinates 1e-3 px, scores 1e-5, plus finite,
in-bounds outputs.  The fine level is fed the kernel's own mid matches.  tests/test_regress_range_emulated.py runs the
same cases on the kernels' code on the CPU; the case tables and the yardstick are in tests/range_reference.py.

contrast and reparam are asserted at the bars up to 2^16 and REPORTED at 2^20, 2^24, 2^28 (one printed line per case
and mode, pytest -s; the cap is range_reference.cap).  DESIGN.md, "Numeric domain of the fp16x2 paths", holds the table."""
import pytest
import torch

import golden_util as gu
import range_reference as rr
import stress_inputs as si
from oracle import p2p_oracle as orc
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu

H, W, N = 96, 128, 64
MODES = ["fp16x2", "fp16x2w", "f32"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from patch2pix_amd import ops
    return ops


def _weights(ops, sd, mode, dev):
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    mid, fine = ops.RegressorWeights(sub("regress_mid."), dev), ops.RegressorWeights(sub("regress_fine."), dev)
    mid.set_mode(mode)
    fine.set_mode(mode)
    return mid, fine


@pytest.fixture(scope="module")
def base_weights(dev, ops):
    return {mode: _weights(ops, gu.state_dict(0), mode, dev) for mode in MODES}


def _gpu(pyr, dev):
    return [t.to(dev) for t in pyr]


def _cpu(out):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _report(name, mode, res, tag="range"):
    print(f"\n{tag}[MI355X] {name:>20s} {mode:>8s}: coord {res['coord']:.2e} px  score {res['score']:.2e}  raw {res['raw']:.2e}"
          f"  | fp32 oracle: {res['o32_coord']:.2e} px  {res['o32_score']:.2e}  {res['o32_raw']:.2e}")


def _pyramid_case(name, mode, dev, ops, base_weights, H=H, W=W, N=N, tag="range"):
    p1, p2 = rr.pair(name, H, W)
    props = rr.proposals(H, W, N)
    mid_w, fine_w = base_weights[mode]
    out = _cpu(ops.regress(mid_w, fine_w, _gpu(p1, dev), _gpu(p2, dev), props.to(dev), want_mid=True, want_raw=True))
    res = rr.measure(out, gu.state_dict(0), p1, p2, props, with_f32=True)
    _report(name, mode, res, tag)
    return res


def _checkpoint_case(name, mode, dev, ops, H=H, W=W, N=N, tag="range"):
    p1, p2 = rr.pair("plain", H, W)
    props = rr.proposals(H, W, N)
    sd = rr.checkpoint(name, p1, p2, props)
    mid_w, fine_w = _weights(ops, sd, mode, dev)
    out = _cpu(ops.regress(mid_w, fine_w, _gpu(p1, dev), _gpu(p2, dev), props.to(dev), want_mid=True, want_raw=True))
    res = rr.measure(out, sd, p1, p2, props, with_f32=True)
    _report(name, mode, res, tag)
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rr.MANDATORY_PYRAMIDS)
def test_pyramid_families_at_the_bars(name, mode, dev, ops, base_weights):
    res = _pyramid_case(name, mode, dev, ops, base_weights)
    assert res["coord"] <= rr.COORD_TOL and res["score"] <= rr.SCORE_TOL, res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rr.MANDATORY_CHECKPOINTS)
def test_checkpoint_families_at_the_bars(name, mode, dev, ops):
    if name.startswith(("reparam", "octaves")):        # the reference does not see these re-parametrisations at all
        p1, p2 = rr.pair("plain", H, W)
        props = rr.proposals(H, W, N)
        assert torch.equal(rr.reference64(rr.checkpoint(name, p1, p2, props), p1, p2, props)[2],
                           rr.reference64(gu.state_dict(0), p1, p2, props)[2])
    res = _checkpoint_case(name, mode, dev, ops)
    assert res["coord"] <= rr.COORD_TOL and res["score"] <= rr.SCORE_TOL, res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("octaves", rr.REPORTED_OCTAVES)
@pytest.mark.parametrize("family", ["contrast_half", "contrast_checker", "reparam"])
def test_reported_beyond_the_mandatory_line(family, octaves, mode, dev, ops, base_weights):
    """Reported, not asserted at the bars in the two-plane modes: finite, in-bounds outputs (rr.measure) and no more than
    cap(k) = 2^(k - 16) times the bars (derivation: range_reference.cap).  Mode f32 is the control: at the bars, for every k."""
    name = f"{family}{octaves}"
    res = _checkpoint_case(name, mode, dev, ops) if family == "reparam" else _pyramid_case(name, mode, dev, ops, base_weights)
    f = rr.reported_factor(octaves, mode)
    assert res["coord"] <= rr.COORD_TOL * f and res["score"] <= rr.SCORE_TOL * f, res


@pytest.mark.parametrize("mode", ["fp16x2w", "fp16x2"])
@pytest.mark.parametrize("octaves", (16,) + rr.REPORTED_OCTAVES)
@pytest.mark.parametrize("family", ["contrast_half", "reparam"])
def test_emulator_configuration_on_the_gpu(family, octaves, mode, dev, ops, base_weights):
    """The inputs of tests/test_regress_range_emulated.py themselves (48 x 64, its three proposals) on the MI355X, one
    printed line per case ("same-input[MI355X]"): next to that file's "range[emulator]" line of the same case the two
    figures say whether the stand-in's fp16 arithmetic -- subnormal low planes beyond 2^17 above all -- is the hardware's
    ("Numeric domain of the fp16x2 paths", third column).  Same bounds as the case has everywhere else."""
    name = f"{family}{octaves}"
    kw = dict(H=48, W=64, N=3, tag="same-input")
    res = _checkpoint_case(name, mode, dev, ops, **kw) if family == "reparam" else _pyramid_case(name, mode, dev, ops, base_weights, **kw)
    f = rr.reported_factor(octaves, mode)
    assert res["coord"] <= rr.COORD_TOL * f and res["score"] <= rr.SCORE_TOL * f, res


@pytest.mark.parametrize("mode", MODES)
def test_stress_items_do_not_change_their_batch_mates(mode, dev, ops, base_weights):
    """ops.regress_batch with stress and ordinary items mixed in ONE launch: the scratch buffer and the persistent
    work-groups are shared between the items, the exponents must not be.  Every item -- the ordinary ones beside a dead
    or a high-contrast one, and those themselves -- has the bits of its single launch, and meets the bars."""
    names = ["plain", "dead_level0", "contrast_half16", "plain", "contrast_checker16", "dead", "global-24", "global+24"]
    mid_w, fine_w = base_weights[mode]
    pairs = [tuple(rr.PYRAMIDS[n][0](40 + 2 * i + s, H, W) for s in (0, 1)) for i, n in enumerate(names)]
    props = [rr.proposals(H, W, N, seed=20 + i) for i in range(len(names))]
    g1, g2 = [_gpu(p[0], dev) for p in pairs], [_gpu(p[1], dev) for p in pairs]
    outs = ops.regress_batch(mid_w, fine_w, g1, g2, [p.to(dev) for p in props], want_mid=True, want_raw=True)
    outs = [_cpu(o) for o in outs]
    for i, n in enumerate(names):
        single = _cpu(ops.regress(mid_w, fine_w, g1[i], g2[i], props[i].to(dev), want_mid=True, want_raw=True))
        for k, v in single.items():
            assert torch.equal(outs[i][k], v), f"item {i} ({n}), {k}: the batch changes it by {float((outs[i][k] - v).abs().max()):.3e}"
        res = rr.measure(outs[i], gu.state_dict(0), pairs[i][0], pairs[i][1], props[i])
        assert res["coord"] <= rr.COORD_TOL and res["score"] <= rr.SCORE_TOL, (n, res)


def test_mixed_regime_end_to_end(dev):
    """model_helper.load_model on a checkpoint whose regressors are neg_gamma o octaves, predict_fine_from_feats on a
    contrast(2^12) pair: the coarse rows of the kernel through the fp64 reference's two levels -- two orc.fine_level calls
    in fp64, which is what orc.predict_fine does behind its coarse stage, but in fp64 and on the kernel's rows (predict_fine
    takes no rows).  The near-integer exclusion applies to the fine level only.  Rows whose reference mid
    coordinate is within 2e-4 px of an integer may move by one patch pixel (trunc, networks/utils.py:19): at most two."""
    from patch2pix_amd.utils.eval import model_helper
    from test_gpu_parity import _near_integer_rows
    Hh, Ww = 128, 160
    q1, q2 = synthetic.make_correlated_pyramids(41, Hh, Ww)
    p1, p2 = si.contrast_of(q1, 12), si.contrast_of(q2, 12)
    f1, f2 = [t[None].to(dev) for t in p1], [t[None].to(dev) for t in p2]
    ckpt = synthetic.make_checkpoint(0)
    with torch.no_grad():
        coarse = model_helper.load_model(ckpt, lprint=lambda *a: None).predict_fine_from_feats(f1, f2, return_all=True)[4][0].cpu()
    assert coarse.shape[0] >= 40
    sd = rr.recentre(si.neg_gamma(si.octaves(ckpt["state_dict"])), p1[:4], p2[:4], coarse)
    net = model_helper.load_model(dict(ckpt, state_dict=sd), lprint=lambda *a: None)
    with torch.no_grad():
        fine, fine_scores, mid, mid_scores, coarse2 = net.predict_fine_from_feats(f1, f2, return_all=True)
    torch.cuda.synchronize()
    assert torch.equal(coarse2[0].cpu(), coarse)
    d = lambda p: [t.double() for t in p[:4]]
    mid_p, fine_p = rr.params64(sd)
    with torch.no_grad():
        ref_mid, ref_mp, ref_raw = orc.fine_level(d(p1), d(p2), coarse, mid_p)
        ref_fine, ref_fp, ref_raw2 = orc.fine_level(d(p1), d(p2), ref_mid, fine_p)
    assert min(rr.sensitive_fraction(ref_raw, ref_mid, Ww, Hh), rr.sensitive_fraction(ref_raw2, ref_fine, Ww, Hh)) >= 0.3
    err = lambda a, b: (a.cpu().double() - b).abs().max().item()
    ok = ~_near_integer_rows(ref_mid)
    print(f"\nmixed regime: {coarse.shape[0]} rows, mid {err(mid[0], ref_mid):.2e} px / {err(mid_scores[0], ref_mp):.2e}, "
          f"fine {err(fine[0].cpu()[ok], ref_fine[ok]):.2e} px / {err(fine_scores[0].cpu()[ok], ref_fp[ok]):.2e}, {int((~ok).sum())} near-integer row(s)")
    assert int((~ok).sum()) <= 2
    assert err(mid[0], ref_mid) <= rr.COORD_TOL and err(mid_scores[0], ref_mp) <= rr.SCORE_TOL
    assert err(fine[0].cpu()[ok], ref_fine[ok]) <= rr.COORD_TOL and err(fine_scores[0].cpu()[ok], ref_fp[ok]) <= rr.SCORE_TOL
