"""TEST INFRASTRUCTURE: what the tests of the generic regressor's second arithmetic (P2P_REGRESS_GENERIC_FP16X2,
csrc/regress_generic_h2.hip) share, on top of tests/regressor_reference.py: the mode ids, handles of a case in a mode through
the C ABI of the emulator's library, the two "range" variants of a case's checkpoint, and the restatement of such a variant at
the project's bars (COORD_TOL / SCORE_TOL, with the conditioning check COND_COORD / COND_SCORE of the inputs)."""
import torch

import regressor_reference as rr

GENERIC, GENERIC_FP16X2 = 16, 17
OK, EINVAL, EUNSUPPORTED, ENOMEM = 0, -1, -3, -4
TUNED_IDS = (0, 3, 4, 5)

# name -> what happens to layer 0's BatchNorm of BOTH regressors of the case
#   up / down: weight and bias x 2^10 / 2^-10 -- every value the layer stores moves by the same factor, so the per-sample exponent
#              of the next layer sits 10 binades away from where the synthetic checkpoint puts it, at either end
#   outlier:   the weight of ONE channel x 2^8 -- that channel sets the sample's exponent, the others lie 8 binades below it
VARIANTS = ("up", "down", "outlier")
# The outlier's channel plays the part of a seed: a weight x 2^8 drives most of case A's outputs into a region where the fp32
# restatement itself is more than COND_* from its fp64 evaluation (coordinates flip by whole pixels).  Of the 64 channels, 3, 32
# and 60 pass the conditioning check on both input sets (test_generic_mode_host.py); 60 is the one that leaves coordinate offsets
# over the whole [-8, 8) range on the "gpu" inputs (the scores saturate at 1 for all three).
OUTLIER_CHANNEL = 60


def variant_state_dict(case, variant):
    """A fresh state_dict of the case's checkpoint with layer 0's BatchNorm changed (the shared checkpoint stays as it is)."""
    sd = {k: v.clone() for k, v in rr.checkpoint(case)["state_dict"].items()}
    for prefix in ("regress_mid.", "regress_fine."):
        w, b = sd[prefix + "conv.1.weight"], sd[prefix + "conv.1.bias"]
        if variant == "up":
            w *= 2.0 ** 10; b *= 2.0 ** 10
        elif variant == "down":
            w *= 2.0 ** -10; b *= 2.0 ** -10
        elif variant == "outlier":
            w[OUTLIER_CHANNEL] *= 2.0 ** 8
        else:
            raise KeyError(variant)
    return sd


def variant_params(case, variant, dtype=torch.float32):
    sd = variant_state_dict(case, variant)
    return rr.sub_params(sd, "regress_mid.", dtype), rr.sub_params(sd, "regress_fine.", dtype)


def levels_of(params, pyr1, pyr2, props, case, mid_out=None):
    """(mid matches, mid probs, fine matches, fine probs) of the restatement in the dtype of `params`; the fine level starts from
    mid_out when given (the kernel's own mid matches, as rr.check_levels does), else from the restatement's."""
    dt = params[0]["conv.0.weight"].dtype
    q1, q2 = rr.to_dtype(pyr1, dt), rr.to_dtype(pyr2, dt)
    m1, s1, _ = rr.fine_level(q1, q2, props, params[0], case)
    m2, s2, _ = rr.fine_level(q1, q2, m1 if mid_out is None else mid_out, params[1], case)
    return m1, s1, m2, s2


def check_variant(out, pyr1, pyr2, props, case, variant, label=""):
    """A variant's outputs at the bars of rr.check_levels (whose restatement reads the unmodified checkpoint), after the
    conditioning check of these inputs: the fp32 restatement within COND_* of its own fp64 evaluation, both levels, the fine level
    of both started from the kernel's mid matches."""
    mid = out["matches1"].cpu()
    p32, p64 = variant_params(case, variant), variant_params(case, variant, torch.float64)
    r32 = levels_of(p32, pyr1, pyr2, props, case, mid_out=mid)
    r64 = levels_of(p64, pyr1, pyr2, props, case, mid_out=mid.double())
    cond = [(a.double() - b).abs().max().item() for a, b in zip(r32, r64)]
    print(f"case {case} variant {variant} {label}: conditioning coord {max(cond[0], cond[2]):.3g} px score {max(cond[1], cond[3]):.3g}")
    assert max(cond[0], cond[2]) <= rr.COND_COORD and max(cond[1], cond[3]) <= rr.COND_SCORE, cond
    errs = [(out[k].cpu() - r).abs().max().item() for k, r in zip(("matches1", "probs1", "matches2", "probs2"), r32)]
    print(f"case {case} variant {variant} {label}: mid coord {errs[0]:.3g} px score {errs[1]:.3g}, fine coord {errs[2]:.3g} px score {errs[3]:.3g}")
    assert errs[0] <= rr.COORD_TOL and errs[2] <= rr.COORD_TOL and errs[1] <= rr.SCORE_TOL and errs[3] <= rr.SCORE_TOL, errs
    return errs


def emu_handles(emu, case, mode=GENERIC_FP16X2, sd=None):
    """(mid, fine) generic handles of a case (of `sd` when given) in `mode`, through the emulator library's C ABI."""
    sd = rr.checkpoint(case)["state_dict"] if sd is None else sd
    out = []
    for prefix in ("regress_mid.", "regress_fine."):
        st, h = rr.create_config(emu, rr.sub_params(sd, prefix), rr.CASES[case])
        assert st == OK, emu.p2p_last_error()
        assert emu.p2p_regressor_get_mode(h) == GENERIC
        assert emu.p2p_regressor_set_mode(h, mode) == OK, emu.p2p_last_error()
        assert emu.p2p_regressor_get_mode(h) == mode
        out.append(h)
    return out


def destroy(emu, *handles):
    for h in handles:
        emu.p2p_regressor_destroy(h)
