"""TEST INFRASTRUCTURE: what the tests of the generic consensus net's second arithmetic (P2P_COARSE_GENERIC_FP16X2,
csrc/consensus_generic_h2.hip) share, on top of tests/ncn_reference.py: tests/test_ncn_mode_host.py, test_ncn_mode_emulated.py,
test_gpu_ncn_mode.py and the fixture generator tests/make_golden_ncn_mode.py.

Inputs beyond those of ncn_reference:
  * volume "tile" (2, 2, 5, 5, 19): the mode's kernel tiles wA and hB by 4 and wB by 16 (the exact kernel wB by 16), so every tiled
    axis is one full tile plus a partial one -- more than one row tile and more than one work-group, which none of the volumes
    REF_ERR was measured on has;
  * range variants of the cases with a hidden layer: "up" / "down" (layer 0's weight and bias x 2^+-10: the hidden volume the
    mode rescales moves by the same factor) and "outlier" (one hidden channel of layer 0 x 2^8: one channel sets the pair's
    scale, the others sit eight bits lower), the channel picked from the fp64 restatement alone as the first that leaves at least
    nr.MIN_SHARE of the cells of "big" alive behind the last ReLU;
  * a mixed batch: the pairs of "big" scaled by 1, 2^12 and 2^-12.
Bars are the project's (nr.BAR_F64 / nr.BAR_GOLDEN x the reference's own fp32 error), per PAIR: an output is compared with the
largest fp64 value of its own pair (nr.check takes the batch's, which would hide an error that scales with the batch).  The
reference's error of an input is max(nr.REF_ERR[case], what tests/make_golden_ncn_mode.py measured per pair on that input):
REF_ERR_MODE below is that script's printed table.  Nothing here is derived from the kernel's output."""
import os

import numpy as np
import torch

import ncn_reference as nr

HERE = os.path.dirname(os.path.abspath(__file__))

GENERIC, GENERIC_FP16X2 = 0, 17
OK, EINVAL, EHIP, EUNSUPPORTED, ENOMEM = 0, -1, -2, -3, -4

TILE = "tile"
VOLUMES = {**nr.VOLUMES, TILE: (2, 2, 5, 5, 19)}
VARIANTS = ("up", "down", "outlier")
HIDDEN_CASES = ("R", "N", "P", "M")
MIXED_FACTORS = (1.0, 2.0 ** 12, 2.0 ** -12)

# (case, input) -> the reference's fp32 error per pair, max |ref32 - f64| / max |f64 of the pair|, where it exceeds
# nr.REF_ERR[case]; inputs: a volume name, or "<variant>:<volume>" (tests/make_golden_ncn_mode.py prints this table)
REF_ERR_MODE = {("R", "up:big"): 5.37e-07, ("R", "up:tile"): 5.46e-07, ("R", "outlier:big"): 5.65e-07, ("R", "mixed"): 6.58e-07,
                ("N", "big"): 4.16e-07, ("N", "outlier:big"): 4.3e-07, ("N", "outlier:tile"): 3.84e-07, ("N", "mixed"): 3.77e-07,
                ("P", "big"): 1.64e-06, ("P", "outlier:big"): 1.47e-06, ("M", "big"): 4.09e-07, ("M", "thin"): 3.9e-07,
                ("M", "tile"): 7.6e-07, ("M", "up:big"): 4.25e-07, ("M", "up:tile"): 8.12e-07, ("M", "outlier:big"): 5.19e-07,
                ("M", "outlier:tile"): 4.4e-07, ("M", "mixed"): 5.16e-07, ("S", "big"): 1.34e-07, ("S", "tile"): 1.31e-07}


def ref_err(case, key):
    return max(nr.REF_ERR[case], REF_ERR_MODE.get((case, key), 0.0))


def golden_name(case):
    return os.path.join(HERE, "golden", f"ncn_mode_{case}.npz")


def load_golden(case):
    return dict(np.load(golden_name(case)))


def volume(name):
    if name in nr.VOLUMES:
        return nr.volume(name)
    shape = VOLUMES[name]
    fa, fb = nr.features(7000 + sum(shape), shape)
    fa = fa / (fa.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    fb = fb / (fb.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    return nr.mutual_matching(torch.einsum("bcij,bckl->bijkl", fa, fb)).contiguous()


_cache = {}


def outlier_channel(case):
    """The first hidden channel of layer 0 whose x 2^8 leaves nr.MIN_SHARE of the cells of "big" alive (fp64 restatement alone)."""
    key = ("outlier", case)
    if key not in _cache:
        x = nr.volume("big")
        for ch in range(nr.CASES[case]["channels"][0]):
            y = nr.restate(x, _scaled(nr.weights(case), ch, 2.0 ** 8), nr.CASES[case])
            if float((y > 0).double().mean()) >= nr.MIN_SHARE:
                _cache[key] = ch
                break
        else:
            raise AssertionError(f"case {case}: no hidden channel keeps {nr.MIN_SHARE} of the cells alive")
    return _cache[key]


def _scaled(sd, ch, factor):
    sd = {k: v.clone() for k, v in sd.items()}
    if ch is None:
        sd["conv.0.weight"] *= factor
        sd["conv.0.bias"] *= factor
    else:
        sd["conv.0.weight"][:, ch] *= factor          # stored layout [k, c_out, c_in, k, k, k]
        sd["conv.0.bias"][ch] *= factor
    return sd


def weights(case, variant=None):
    sd = nr.weights(case)
    if variant is None:
        return sd
    assert case in HIDDEN_CASES and variant in VARIANTS
    if variant == "outlier":
        return _scaled(sd, outlier_channel(case), 2.0 ** 8)
    return _scaled(sd, None, 2.0 ** (10 if variant == "up" else -10))


def expected(case, vol, variant=None):
    """(x fp32, y fp64), computed once and shared; callers must not modify them."""
    if variant is None and vol in nr.VOLUMES:
        return nr.expected(case, vol)
    key = (case, vol, variant)
    if key not in _cache:
        x = volume(vol)
        _cache[key] = (x, nr.restate(x, weights(case, variant), nr.CASES[case]))
    return _cache[key]


def mixed(case):
    """(x fp32, y fp64): the three pairs of "big" at magnitudes 2^12 apart."""
    key = (case, "mixed")
    if key not in _cache:
        x = nr.volume("big") * torch.tensor(MIXED_FACTORS, dtype=torch.float32).view(3, 1, 1, 1, 1)
        _cache[key] = (x, nr.restate(x, nr.weights(case), nr.CASES[case]))
    return _cache[key]


def input_key(vol, variant=None):
    return vol if variant is None else f"{variant}:{vol}"


def check_pairs(out, y64, case, key, label, bar=nr.BAR_F64, ref=None):
    """Per pair: max |out - ref| <= bar x ref_err x max |fp64 of the pair| (`ref`: what to compare with, default the fp64 values);
    prints each figure before it asserts."""
    assert torch.isfinite(out).all(), f"case {case} {key} {label}: non-finite output"
    ref = y64 if ref is None else ref
    worst = []
    for z in range(out.shape[0]):
        scale = y64[z].abs().max().item()
        err = (out[z].double() - ref[z].double()).abs().max().item()
        tol = bar * ref_err(case, key) * scale
        print(f"case {case} input {key} pair {z} {label}: max err {err:.3g} (relative {err / scale if scale else 0.0:.3g}), bar {tol:.3g}")
        worst.append((err, tol))
    for z, (err, tol) in enumerate(worst):
        assert err <= tol, f"case {case} input {key} pair {z} {label}: {err:.3g} > {tol:.3g}"


def handles_bar_pairs(case, y64):
    """nr.handles_bar per pair."""
    return [nr.handles_bar(case, y64[z]) for z in range(y64.shape[0])]


def create(lib, case, variant=None, mode=GENERIC, layout=None):
    """A generic handle of a case on `lib` (the emulated library or the real one) in `mode`."""
    st, h = nr.create_config(lib, weights(case, variant), layout or nr.CASES[case])
    assert st == OK, lib.p2p_last_error()
    assert lib.p2p_ncn_get_mode(h) == GENERIC
    if mode != GENERIC:
        assert lib.p2p_ncn_set_mode(h, mode) == OK, lib.p2p_last_error()
    return h
