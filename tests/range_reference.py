"""The case tables and the fp64 yardstick shared by tests/test_regress_range_emulated.py (the kernels' code on the CPU)
and tests/test_gpu_regress_range.py (the MI355X): which stress inputs (tests/stress_inputs.py) are asserted at the
project's bars, which are reported under a cap, and how a kernel result is measured against orc.fine_level in fp64."""
import torch

import golden_util as gu
import stress_inputs as si
from oracle import p2p_oracle as orc

COORD_TOL, SCORE_TOL = 1e-3, 1e-5              # the project's bars (tests/test_gpu_parity.py)
MANDATORY_OCTAVES = 16                         # contrast / reparam are asserted at the bars up to 2^16

# id -> (function of (seed, H, W), also run in mode f32)
PYRAMIDS = {}
for _k in (-24, -12, 12, 24, 30):        # +30: a norm past 2^31, where a cell exponent clamped too early overflows fp16
    PYRAMIDS[f"global{_k:+d}"] = (lambda s, H, W, k=_k: si.global_scale(s, H, W, k), False)
for _v in ("half", "checker"):
    for _k in (8, 16):
        PYRAMIDS[f"contrast_{_v}{_k}"] = (lambda s, H, W, k=_k, v=_v: si.contrast(s, H, W, k, v), True)
for _lv in (3, 1):
    for _k in (10, -10):
        PYRAMIDS[f"level{_lv}_imbalance{_k:+d}"] = (lambda s, H, W, k=_k, lv=_lv: si.level_imbalance(s, H, W, k, lv), False)
PYRAMIDS["outlier12"] = (lambda s, H, W: si.outlier(s, H, W, 12), False)
PYRAMIDS["dead"] = (lambda s, H, W: si.dead(s, H, W, False), True)
PYRAMIDS["dead_level0"] = (lambda s, H, W: si.dead(s, H, W, True), True)
PYRAMIDS["signed"] = (lambda s, H, W: si.signed(s, H, W), False)
PYRAMIDS["plain"] = (lambda s, H, W: si._base(s, H, W), False)       # the input of the checkpoint cases

# id -> (function of the state_dict, re-centre fc.6.bias, also run in mode f32)
CHECKPOINTS = {
    "reparam8": (lambda sd: si.reparam(sd, 8), False, True),
    "reparam16": (lambda sd: si.reparam(sd, 16), False, True),
    "reparam_all24": (lambda sd: si.reparam(sd, 24, every=1), False, False),      # every |H| far below 1: the exponent of max |H|
    "neg_gamma": (si.neg_gamma, True, True),
    "var_spread": (si.var_spread, True, False),
    "dead_channels": (si.dead_channels, True, False),
    "octaves": (si.octaves, False, False),
}
REPORTED_OCTAVES = (20, 24, 28)                # contrast (half) and reparam beyond the mandatory line
for _k in REPORTED_OCTAVES:
    PYRAMIDS[f"contrast_half{_k}"] = (lambda s, H, W, k=_k: si.contrast(s, H, W, k, "half"), True)
    PYRAMIDS[f"contrast_checker{_k}"] = (lambda s, H, W, k=_k: si.contrast(s, H, W, k, "checker"), True)
    CHECKPOINTS[f"reparam{_k}"] = (lambda sd, j=_k: si.reparam(sd, j), False, True)
MANDATORY_PYRAMIDS = [k for k in PYRAMIDS if k != "plain"
                      and k not in {f"contrast_{v}{j}" for v in ("half", "checker") for j in REPORTED_OCTAVES}]
MANDATORY_CHECKPOINTS = [k for k in CHECKPOINTS if k not in {f"reparam{j}" for j in REPORTED_OCTAVES}]


def pair(name, H, W, seed=7):
    fn = PYRAMIDS[name][0]
    return fn(seed, H, W), fn(seed + 1, H, W)


def proposals(H, W, n, seed=9):
    """Integer proposals [n, 4]: an image corner, one whose two patches straddle the middle column (the edge of the
    'half' region), one inside the top-left 'corner' region, the rest seeded."""
    g = torch.Generator().manual_seed(seed)
    props = torch.stack([torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g),
                         torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g)], 1)
    props[0] = torch.tensor([0, 0, W, H])
    props[1] = torch.tensor([W // 2 + 1, H // 3, W // 2 - 3, H // 2 + 5])
    if n > 2:
        props[2] = torch.tensor([11, 13, W // 2 + 6, 20])
    return props


def params64(sd):
    return orc.split_params(sd, torch.float64)[1:]


def reference64(sd, p1, p2, props):
    """fp64 reference of the mid level: (matches, scores, raw)."""
    d = lambda p: [t.double() for t in p]
    with torch.no_grad():
        return orc.fine_level(d(p1), d(p2), props, params64(sd)[0])


def checkpoint(name, p1, p2, props):
    """The state_dict of a checkpoint case; where the table asks for it, fc.6.bias of both regressors is re-centred on
    the fp64 reference's raw outputs on the caller's own proposals (mid, then fine on the fp64 mid matches)."""
    fn, centre, _ = CHECKPOINTS[name]
    sd = fn(gu.state_dict(0))
    return recentre(sd, p1, p2, props, calm=name == "var_spread") if centre else sd


def recentre(sd, p1, p2, props, calm=False):
    """fc.6.bias of both regressors of `sd` re-centred in place (stress_inputs.recentre; with `calm` after
    stress_inputs.calm) on the fp64 reference's raw outputs on `props`: mid, then fine on the fp64 mid matches."""
    d = lambda p: [t.double() for t in p]

    def settle(prefix, which, matches):
        raw = orc.fine_level(d(p1), d(p2), matches, params64(sd)[which])[2]
        if calm:
            si.calm(sd, prefix, raw.std(dim=0))
            raw = orc.fine_level(d(p1), d(p2), matches, params64(sd)[which])[2]
        si.recentre(sd, prefix, raw.mean(dim=0))
        return orc.fine_level(d(p1), d(p2), matches, params64(sd)[which])[0]
    with torch.no_grad():
        settle("regress_fine.", 1, settle("regress_mid.", 0, props))
    return sd


def sensitive_fraction(raw, matches, W, H):
    """Share of the four offsets 16 tanh(relu(o)) - 8 strictly inside (-8, 8) whose coordinate is not at an image bound."""
    off = 16.0 * torch.tanh(torch.relu(raw[:, :4])) - 8.0
    hi = torch.tensor([W, H, W, H], dtype=matches.dtype)
    ok = (off > -8) & (off < 8) & (matches > 0) & (matches < hi)
    return ok.double().mean().item()


def measure(out, sd, p1, p2, props, with_f32=False):
    """Errors of a kernel result `out` (CPU tensors matches1/probs1/raw1/matches2/probs2/raw2) against the fp64
    reference; the fine level is fed the kernel's own mid matches (a last-bit wobble across an integer would move the
    whole fine patch, networks/utils.py:19).  Asserts finite, in-bounds outputs and that the case is a sensitive one.
    -> dict coord / score / raw (+ o32_* : the fp32 oracle's own error on the same inputs)."""
    H, W = p1[0].shape[1:]
    d = lambda p: [t.double() for t in p]
    mid_p, fine_p = params64(sd)
    with torch.no_grad():
        r1 = orc.fine_level(d(p1), d(p2), props, mid_p)
        r2 = orc.fine_level(d(p1), d(p2), out["matches1"].double(), fine_p)
    hi = torch.tensor([W, H, W, H], dtype=torch.float32)
    for lvl in ("1", "2"):
        m, p = out["matches" + lvl], out["probs" + lvl]
        assert torch.isfinite(m).all() and torch.isfinite(p).all() and torch.isfinite(out["raw" + lvl]).all()
        assert (m >= 0).all() and (m <= hi).all() and (p >= 0).all() and (p <= 1).all()
    f1 = sensitive_fraction(r1[2], r1[0], W, H)
    f2 = sensitive_fraction(r2[2], r2[0], W, H)
    assert min(f1, f2) >= 0.3, f"only {f1:.2f} / {f2:.2f} of the reference's offsets are off the clamp bounds"
    err = lambda a, b: (a.double() - b).abs().max().item()
    res = {"coord": max(err(out["matches1"], r1[0]), err(out["matches2"], r2[0])),
           "score": max(err(out["probs1"], r1[1]), err(out["probs2"], r2[1])),
           "raw": max(err(out["raw1"], r1[2]), err(out["raw2"], r2[2]))}
    if with_f32:
        m32, f32p = orc.split_params(sd)[1:]
        with torch.no_grad():
            o1 = orc.fine_level(p1, p2, props, m32)
            o2 = orc.fine_level(p1, p2, out["matches1"], f32p)
        res.update(o32_coord=max(err(o1[0], r1[0]), err(o2[0], r2[0])), o32_score=max(err(o1[1], r1[1]), err(o2[1], r2[1])),
                   o32_raw=max(err(o1[2], r1[2]), err(o2[2], r2[2])))
    return res


def reported_factor(octaves, mode):
    """Factor over the bars a reported case is held to: cap(octaves) in the two-plane modes; 1 in mode f32, which has no
    planes to lose and is the control that shows the growth is theirs."""
    return 1.0 if mode == "f32" else cap(octaves)


def cap(octaves):
    """Factor over the bars that a reported case may reach.  Under a shared exponent an operand 2^k below the largest
    one of its tensor is carried as h0 + h1 with h1 an fp16 subnormal once k > 17: its absolute error is half the
    subnormal spacing, 2^-25 on the scaled value (largest operand in [2^12, 2^13)), i.e. a RELATIVE error of about
    2^(k - 37) -- one bit of the low plane lost per octave, against the 2^-24 both planes carry while they are normal.
    Where that operand is re-normalised afterwards (the per-pixel L2 scale; a conv2 column that is large where its H
    channel is small) the relative error reaches the output, so the error of the case at 2^16, which meets the bars,
    may grow by 2^(k - 16) and no more."""
    return 2.0 ** max(0, octaves - MANDATORY_OCTAVES)
