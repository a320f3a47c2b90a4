"""Mode 'fp16' (P2P_REGRESS_FP16: one fp16 plane per operand, one MFMA per product) -- the case table, the error model its bars
come from, the values measured under emulation, and the helpers shared by tests/test_fast_mode_host.py,
tests/test_fast_mode_emulated.py (the kernels' code on the CPU, tests/hipemu) and tests/test_gpu_fast_mode.py (the MI355X).

The yardstick is the fp64 evaluation of tests/range_reference.py (orc.fine_level) on the stress inputs of
tests/stress_inputs.py; the fine level is fed the kernel's own mid matches (range_reference.measure).

ERROR MODEL (first order, from the operands, in the manner of oracle/error_model.py).  The mode rounds every operand of the
two convolutions ONCE to fp16 under an exact power-of-two scale: relative error |d| <= u = 2^-11, taken as independent with
variance <= u^2 / 3 (uniform over the rounding interval at the bottom of a binade: the largest relative variance).  The
rounding sites are
  a  the conv1 activations (K = 9 * 518 terms per output): the L2-normalised level-0 pixel values, and the cells of levels
     1-3 -- a cell is rounded once (x 2^e of its image) and then serves every patch pixel it covers, so its error is ONE
     variable for all of them (gradients are summed per cell before they are squared; border clamping included);
  w  the conv1 weights (per output channel scale);
  U  the Winograd-transformed conv2 input B^T d B (K = 9 * 512 terms per output in the direct form; 16 positions x 512 here);
  W  the transformed filters G g G^T, rounded once from fp64.
Everything else (gather, L2 norm, BatchNorm folds, output transform, ReLU / max-pool, FC tail, parse_regressor_out) is the fp32
code of the default mode, which is held to COORD_TOL / SCORE_TOL: those bars are ADDED as the floor of the model.
To first order the raw output o_j moves by sum_s (do_j / ds) s d_s over all sites s, so
    var(o_j) <= (u^2 / 3) * sum_s (s * do_j / ds)^2,
with the gradients taken by autograd on an fp64 evaluation that computes conv2 in its Winograd form (winograd_forward;
asserted equal to the direct form).  The bound on a raw output is LAM standard deviations; it goes through
parse_regressor_out by the largest slope of psize * tanh(relu(.)) over the interval (at most 16) and of the sigmoid (1 / 4).
LAM = 6: a Gaussian tail of 2e-9 per output, against a few hundred asserted outputs.

MEASURED (emulated kernels, this table, max over proposals and both levels) next to the model's bound: MEASURED_EMULATED below;
the same table is in DESIGN.md section 4, "Single-plane mode".  The tests assert the MODEL's bound, never a measured value."""
import ctypes

import torch
import torch.nn.functional as F

import range_reference as rr
from oracle import p2p_oracle as orc

MODE = "fp16"
MODE_ID = 5                      # P2P_REGRESS_FP16 (include/p2p_hip.h)
U_FP16 = 2.0 ** -11              # relative rounding of one fp16 operand
LAM = 6.0
IO_THRES = 0.25                  # the reference's io_thres: a proposal whose score crosses it changes side
H, W, N = 48, 64, 3              # the emulated table: 48 x 64 pyramids, rr.proposals (corner, across the region edge, dead corner)

# id -> (kind, name in range_reference's tables): feature contrast, weight regimes, border proposals (rr.proposals puts one
# proposal on an image corner in every case: clamped patches)
CASES = {
    "plain": ("pyramid", "plain"),                  # the default family (also measured against the fp32 oracle)
    "contrast_half8": ("pyramid", "contrast_half8"),
    "contrast_checker16": ("pyramid", "contrast_checker16"),
    "outlier12": ("pyramid", "outlier12"),
    "signed": ("pyramid", "signed"),
    "octaves": ("checkpoint", "octaves"),
    "neg_gamma": ("checkpoint", "neg_gamma"),
    "var_spread": ("checkpoint", "var_spread"),
}

# Measured under emulation (tests/test_fast_mode_emulated.py -s prints these lines): max |error| against fp64 over the case's
# proposals and both levels, next to the model's bound for the same proposals.  coord in px, score = io_prob.
MEASURED_EMULATED = {
    #                      coord     bound     score     bound      (fp32 oracle on the same inputs: <= 1.8e-5 px, 2.9e-7)
    "plain":              (8.10e-3, 5.59e-2, 1.64e-4, 1.03e-3),
    "contrast_half8":     (8.10e-3, 5.59e-2, 1.64e-4, 1.03e-3),     # exact power-of-two rescalings: the same bits as plain
    "contrast_checker16": (8.06e-3, 5.59e-2, 1.64e-4, 1.03e-3),
    "outlier12":          (8.22e-3, 5.58e-2, 1.67e-4, 1.03e-3),
    "signed":             (8.04e-3, 5.79e-2, 1.26e-4, 9.84e-4),
    "octaves":            (8.10e-3, 5.59e-2, 1.64e-4, 1.03e-3),
    "neg_gamma":          (9.87e-3, 4.89e-2, 7.84e-5, 8.58e-4),
    "var_spread":         (1.15e-2, 6.71e-2, 8.02e-5, 1.17e-3),
    # also measured, not in the table: contrast_checker8 8.10e-3 / 1.64e-4, level3_imbalance+10 6.02e-3 / 1.25e-4,
    # reparam8 8.10e-3 / 1.64e-4.  Measured / bound = 0.14 ... 0.20 (coord), 0.07 ... 0.17 (score).
}


def case_inputs(name, h=H, w=W, n=N):
    kind, key = CASES[name]
    props = rr.proposals(h, w, n)
    import golden_util as gu
    if kind == "pyramid":
        p1, p2 = rr.pair(key, h, w)
        sd = gu.state_dict(0)
    else:
        p1, p2 = rr.pair("plain", h, w)
        sd = rr.checkpoint(key, p1, p2, props)
    return sd, p1, p2, props


def unrounded_pair(hh, ww, seed=3):
    """Pyramids of an image whose size is no multiple of 8, as the backbone makes them: level j has ceil(dim / 2^j) rows and
    columns (the gather clamps to dim // 2^j - 1, networks/utils.py:22-23; tests/test_kernels_emulated.py has the same maps)."""
    gen = torch.Generator().manual_seed(seed)
    up = lambda d, j: (d + (1 << j) - 1) >> j
    pyr = lambda: [torch.randn(3, hh, ww, generator=gen)] + [torch.relu(torch.randn(c, up(hh, j), up(ww, j), generator=gen) + 0.3)
                                                             for c, j in ((64, 1), (64, 2), (128, 3))]
    return pyr(), pyr()


# ------------------------------------------------------------------------------------------------ handles (emulator or library)
def sub_sd(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def create(lib, sub, mode_id):
    """A tuned regressor handle of `lib` (the emulated or the real library) in mode `mode_id`; -> (handle, keep-alive)."""
    from patch2pix_amd import _lib as real
    keep = {k: v.detach().float().contiguous() for k, v in sub.items() if v.is_floating_point()}
    p = real.RegressorParams()
    bn = lambda q: real.BnParams(keep[q + ".weight"].data_ptr(), keep[q + ".bias"].data_ptr(),
                                 keep[q + ".running_mean"].data_ptr(), keep[q + ".running_var"].data_ptr())
    p.conv1_w = keep["conv.0.weight"].data_ptr(); p.bn1 = bn("conv.1")
    p.conv2_w = keep["conv.2.weight"].data_ptr(); p.bn2 = bn("conv.3")
    p.fc1_w = keep["fc.0.weight"].data_ptr(); p.fc1_b = keep["fc.0.bias"].data_ptr(); p.bnf1 = bn("fc.1")
    p.fc2_w = keep["fc.3.weight"].data_ptr(); p.fc2_b = keep["fc.3.bias"].data_ptr(); p.bnf2 = bn("fc.4")
    p.fc3_w = keep["fc.6.weight"].data_ptr(); p.fc3_b = keep["fc.6.bias"].data_ptr()
    h = ctypes.c_void_p()
    assert lib.p2p_regressor_create(ctypes.byref(p), ctypes.byref(h)) == 0, lib.p2p_last_error().decode()
    st = lib.p2p_regressor_set_mode(h, mode_id)
    assert st == 0, f"p2p_regressor_set_mode({mode_id}) returned {st}: {lib.p2p_last_error().decode()}"
    return h, keep


def emu_run(emu, sd, p1, p2, props, mode_id=MODE_ID, two=True, ws_bytes=None):
    """mid (-> fine) through the emulator in mode `mode_id` -> rr.measure's dict of CPU tensors."""
    import regressor_reference as rg
    mid, k1 = create(emu, sub_sd(sd, "regress_mid."), mode_id)
    fine, k2 = create(emu, sub_sd(sd, "regress_fine."), mode_id) if two else (None, None)
    try:
        return rg.emu_regress(emu, mid, fine, p1, p2, props, ws_bytes=ws_bytes)
    finally:
        emu.p2p_regressor_destroy(mid)
        if fine:
            emu.p2p_regressor_destroy(fine)


# ------------------------------------------------------------------------------------------------ the model
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def winograd_forward(z, p, w1, wt):
    """The regressor on one patch z [1, 518, 16, 16] (fp64) with conv2 as Winograd F(2x2, 3x3): w1 = conv.0.weight,
    wt = G g G^T [512, 512, 4, 4].  -> (raw [5], U) with U = B^T d B [1, 512, 4, 4, 4, 4] (tile y, tile x, i, j)."""
    h = orc._bn(F.conv2d(z, w1, None, stride=2, padding=1), p, "conv.1", (1, -1, 1, 1))
    d = F.pad(h, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
    u = torch.einsum("ia,nctxab,jb->nctxij", _BT, d, _BT)
    m = torch.einsum("nctxij,ocij->notxij", u, wt)
    y = torch.einsum("ai,notxij,bj->notxab", _AT, m, _AT)
    y = orc._bn(y, p, "conv.3", (1, -1, 1, 1, 1, 1))
    v = F.relu(y).amax(dim=(2, 3, 4, 5))
    v = F.relu(orc._bn(F.linear(v, p["fc.0.weight"], p["fc.0.bias"]), p, "fc.1", (1, -1)))
    v = F.relu(orc._bn(F.linear(v, p["fc.3.weight"], p["fc.3.bias"]), p, "fc.4", (1, -1)))
    return F.linear(v, p["fc.6.weight"], p["fc.6.bias"])[0], u


def transformed_filters(w2):
    return torch.einsum("ia,ocab,jb->ocij", _G, w2, _G)


def _cell_ids(pyr, x, y):
    """[518 / 2 = 259 channels of one image] -> per level the id of the cell each of the 16 x 16 patch pixels reads
    (networks/utils.py:22-23: index dim // ds - 1 at most), [16, 16] int64."""
    hh, ww = pyr[0].shape[1:]
    off = torch.arange(16) - 8
    ids = []
    for j in range(4):
        ds = 1 << j
        iy = torch.div(y + off, ds, rounding_mode="floor").clamp(0, hh // ds - 1)
        ix = torch.div(x + off, ds, rounding_mode="floor").clamp(0, ww // ds - 1)
        ids.append(iy[:, None] * (ww // ds) + ix[None, :])
    return ids


def raw_std(p1, p2, matches, p):
    """Per proposal the model's standard deviation of the five raw outputs, [n, 5] fp64 (module docstring)."""
    d = lambda q: [t.double() for t in q[:4]]
    p1, p2 = d(p1), d(p2)
    mi = matches.long()
    w1 = p["conv.0.weight"].clone().requires_grad_(True)
    wt = transformed_filters(p["conv.2.weight"]).clone().requires_grad_(True)
    chans = (3, 64, 64, 128)
    out = torch.zeros(matches.shape[0], 5, dtype=torch.float64)
    for i in range(matches.shape[0]):
        f1 = orc.gather_patch_feats(p1, mi[i:i + 1, 0], mi[i:i + 1, 1])
        f2 = orc.gather_patch_feats(p2, mi[i:i + 1, 2], mi[i:i + 1, 3])
        z = torch.cat([f1, f2], 1).clone().requires_grad_(True)
        raw, u = winograd_forward(z, p, w1, wt)
        ids = [_cell_ids(p1, int(mi[i, 0]), int(mi[i, 1])), _cell_ids(p2, int(mi[i, 2]), int(mi[i, 3]))]
        for j in range(5):
            gz, gw1, gwt, gu = torch.autograd.grad(raw[j], (z, w1, wt, u), retain_graph=True)
            var = ((gw1 * w1) ** 2).sum() + ((gwt * wt) ** 2).sum() + ((gu * u) ** 2).sum()
            t = (gz * z).detach()[0]                               # [518, 16, 16]: per unit relative error of each element
            c0 = 0
            for img in range(2):
                for lv in range(4):
                    blk = t[c0:c0 + chans[lv]].reshape(chans[lv], 256)
                    cid = ids[img][lv].reshape(256)
                    uniq, inv = torch.unique(cid, return_inverse=True)
                    s = torch.zeros(chans[lv], uniq.numel(), dtype=torch.float64).index_add_(1, inv, blk)
                    var = var + (s ** 2).sum()
                    c0 += chans[lv]
            out[i, j] = (var.detach() * (U_FP16 ** 2 / 3.0)).sqrt()
    return out


def level_bounds(par, p1, p2, m):
    """The model's bounds for ONE regressor level (fp64 parameters `par`) at the proposals m: per proposal the coordinate
    bound [n] (max over the four coordinates, px) and the score bound [n], WITHOUT the fp32 floor; and the fp64 raw outputs."""
    d = lambda q: [t.double() for t in q[:4]]
    with torch.enable_grad():
        sig = raw_std(p1, p2, m, par)
    with torch.no_grad():
        raw = orc.fine_level(d(p1), d(p2), m, par)[2]
    db = LAM * sig
    lo = torch.relu(raw[:, :4] - db[:, :4])                   # the slope of 16 tanh(relu(o)) is largest at the smallest o >= 0
    slope = 16.0 * (1.0 - torch.tanh(lo) ** 2)
    return (slope * db[:, :4]).amax(1), 0.25 * db[:, 4], raw


def bounds(sd, p1, p2, props, mid_matches):
    """The model's bars for one case: (coord [px], score) = max over the proposals and both levels, the fine level at the
    matches it was actually fed (`mid_matches`, the kernel's own).  Also -> the per-proposal score bounds of the fine level
    (the level whose io_prob is thresholded) and its fp64 scores, for the flip count."""
    mid_p, fine_p = rr.params64(sd)
    coord = score = 0.0
    for par, m in ((mid_p, props), (fine_p, mid_matches.double())):
        cb, sb, raw = level_bounds(par, p1, p2, m)
        coord, score = max(coord, cb.max().item()), max(score, sb.max().item())
        last = (sb, torch.sigmoid(raw[:, 4]))
    return coord + rr.COORD_TOL, score + rr.SCORE_TOL, last[0] + rr.SCORE_TOL, last[1]


def golden_level(tag, n):
    """The reference's own fp32 outputs (tests/golden/fine_48x64.npz, written by the reference's forward_fine_match): tag
    'int_mid' -- integer proposals through the mid regressor -- or 'float_fine' -- float proposals through the fine one.
    -> (pyramid 1, pyramid 2, proposals [n, 4], golden matches, golden probs, fp64 parameters of that regressor).  The golden
    is an fp32 evaluation: its own distance from fp64 is inside the COORD_TOL / SCORE_TOL floor the bars carry."""
    import golden_util as gu
    g = gu.load("fine_48x64")
    p1, p2 = gu.fine_inputs(g)
    par = rr.params64(gu.state_dict(0))[0 if tag == "int_mid" else 1]
    return (p1[:4], p2[:4], torch.from_numpy(g[tag + "_in"][:n]), torch.from_numpy(g[tag + "_matches"][:n]),
            torch.from_numpy(g[tag + "_probs"][:n]), par)


def assert_against_golden(tag, matches, probs, golden, label):
    """`matches` / `probs` of mode fp16 on golden_level(tag, n) within the model's per-proposal bound (+ the fp32 floor) of the
    reference's recorded outputs; prints the figures."""
    p1, p2, props, gm, gp, par = golden
    cb, sb, _ = level_bounds(par, p1, p2, props)
    dc, ds = (matches.double() - gm.double()).abs().amax(1), (probs.double() - gp.double()).abs()
    print(f"\nfp16[{label}] golden fine_48x64 {tag:>10s}: coord {dc.max().item():.2e} px (model {cb.max().item() + rr.COORD_TOL:.2e})  "
          f"score {ds.max().item():.2e} (model {sb.max().item() + rr.SCORE_TOL:.2e})")
    assert bool((dc <= cb + rr.COORD_TOL).all()) and bool((ds <= sb + rr.SCORE_TOL).all()), (dc, cb, ds, sb)
    assert dc.max().item() > rr.COORD_TOL / 10        # (and it is this mode's arithmetic that ran)


def flips(probs, probs64):
    """Proposals on the other side of IO_THRES than the fp64 yardstick."""
    return int(((probs.double() > IO_THRES) != (probs64 > IO_THRES)).sum())


def flip_cap(probs32, probs64, score_bound):
    """What the fp32 reference itself flips on these inputs plus the model's prediction: every proposal whose fp64 score lies
    within its score bound of the threshold may change side."""
    return flips(probs32, probs64) + int(((probs64 - IO_THRES).abs() <= score_bound).sum())
