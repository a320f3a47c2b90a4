"""TEST INFRASTRUCTURE: the cases, seeded inputs, float64 restatements and bars shared by the tests of the operator layer
(networks.modules, networks.ncn.*; csrc/operators.hip and the PLANAR form of csrc/consensus_generic.hip):
tests/test_operators_host.py, test_operators_emulated.py, test_gpu_operators.py and the fixture generator
tests/make_golden_operators.py.

Yardsticks: float64 torch restatements of the reference's operators (the cited lines), and the fixtures
tests/golden/operators_*.npz = the UNMODIFIED reference's own fp32 outputs on the CPU over the same inputs.

Bars (none is derived from a kernel's output):
  equality      pooled values and relocalisation tensors, match indices / coordinates, raw scores: bit for bit with the golden
  MM_BAR        mutual matching: 8 * 2^-24 relative per non-zero element (maximum + eps, two divisions, three multiplications = six
                fp32 roundings, plus second-order terms)
  l2_bar(C)     L2Normalize: (C + 4) * 2^-24 relative (C roundings of the sum at worst, eps, root, division)
  2 x REF_ERR   correlation, Conv4d, NeighConsensus: max |out - f64| / max |f64| against twice the reference's own fp32 error of
                the case, measured by tests/make_golden_operators.py (the tables below, rounded up)
  SOFTMAX_TOL   softmax scores against the golden: the project's 1e-5
"""
import os

import numpy as np
import torch

import ncn_reference as nr
from patch2pix_amd.utils import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- cases ---------------------------------------------------------------------------------------------------------------------
# correlation: (B, C, (hA, wA), (hB, wB)) -- a channel count that is no multiple of 4 x 10, unequal sides that are no multiples
# of the 16 / 64 position tiles; the backbone's 256 channels on more than one work-group per axis; one position against a row
CORR_CASES = {"A": (1, 40, (6, 8), (4, 10)), "B": (2, 256, (16, 20), (16, 20)), "C": (1, 3, (1, 1), (5, 7))}
# 4-D max-pool: k -> [B, H1, W1, H2, W2]
POOL_CASES = {2: (2, 8, 12, 4, 6), 3: (2, 6, 9, 3, 6), 4: (2, 8, 8, 4, 12), 1: (2, 3, 5, 2, 4)}
POOL_VALUES = (-1.5, -0.25, 0.0, 0.5, 2.0)          # five values: most windows hold ties
MM_SHAPE = (2, 5, 6, 4, 7)
# one Conv4d layer: (c_in, c_out, k, bias)
CONV_CASES = {"1to16k3": (1, 16, 3, True), "16to1k3": (16, 1, 3, True), "3to5k5": (3, 5, 5, False)}
CONV_VOLUMES = {"v5674": (2, 5, 6, 4, 7), "v2392": (2, 2, 3, 9, 2)}      # the second: sides below the kernel
# NeighConsensus: the released stack and the class default, symmetric and not
NC_CASES = {"R": dict(kernel_sizes=[3, 3], channels=[16, 1], symmetric_mode=True),
            "Rn": dict(kernel_sizes=[3, 3], channels=[16, 1], symmetric_mode=False),
            "N": dict(kernel_sizes=[3, 3, 3], channels=[10, 10, 1], symmetric_mode=True),
            "Nn": dict(kernel_sizes=[3, 3, 3], channels=[10, 10, 1], symmetric_mode=False)}
NC_SHAPE = (2, 5, 6, 4, 7)
MATCH_SHAPE = (2, 6, 8, 4, 10)
L2_CASES = {"chan": ((2, 40, 6, 8), 1), "first": ((5, 7, 3), 0), "last": ((3, 4, 9), 2)}

MM_BAR = 8 * 2.0 ** -24
SOFTMAX_TOL = 1e-5
BAR = 2.0      # x REF_ERR


def l2_bar(c):
    return (c + 4) * 2.0 ** -24


# max |reference fp32 - fp64| / max |fp64| per case, printed by tests/make_golden_operators.py (rounded up)
REF_ERR = {
    "corr_A": 3e-07, "corr_B": 5.6e-07, "corr_C": 4.64e-08,
    "conv_1to16k3_v5674": 1.34e-07, "conv_1to16k3_v2392": 1.03e-07, "conv_16to1k3_v5674": 4.32e-07, "conv_16to1k3_v2392": 4.91e-07,
    "conv_3to5k5_v5674": 3.35e-07, "conv_3to5k5_v2392": 2.53e-07,
    "nc_R": 2.62e-07, "nc_Rn": 2.9e-07, "nc_N": 3.65e-07, "nc_Nn": 3.78e-07,
}


def golden_name(family):
    return os.path.join(HERE, "golden", f"operators_{family}.npz")


_golden = {}


def golden(family):
    if family not in _golden:
        _golden[family] = dict(np.load(golden_name(family)))
    return _golden[family]


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- seeded inputs (CPU, fp32; callers must not modify them) -------------------------------------------------------------------
_inputs = {}


def _once(key, make):
    if key not in _inputs:
        _inputs[key] = make()
    return _inputs[key]


def corr_inputs(case):
    def make():
        b, c, (ha, wa), (hb, wb) = CORR_CASES[case]
        g = _gen(4100 + ord(case))
        return torch.randn(b, c, ha, wa, generator=g), torch.randn(b, c, hb, wb, generator=g)
    return _once(("corr", case), make)


def pool_input(k):
    def make():
        g = _gen(4200 + k)
        idx = torch.randint(0, len(POOL_VALUES), POOL_CASES[k], generator=g)
        return torch.tensor(POOL_VALUES)[idx].contiguous()
    return _once(("pool", k), make)


def mm_input():
    def make():
        x = torch.rand(MM_SHAPE, generator=_gen(4300))
        x[0, 2, 3] = 0.0          # one A cell with an all-zero slice over B
        x[1, :, :, 1, 5] = 0.0    # and one B cell with an all-zero slice over A
        return x
    return _once("mm", make)


def conv_weights(case):
    def make():
        ci, co, k, bias = CONV_CASES[case]
        g = _gen(4400 + 16 * ci + co + k)
        bound = (6.0 / ((ci + co) * k ** 4)) ** 0.5 * 2.0
        w = (torch.rand(co, ci, k, k, k, k, generator=g) * 2 - 1) * bound
        return w.permute(2, 0, 1, 3, 4, 5).contiguous(), (0.05 * torch.randn(co, generator=g) if bias else None)
    return _once(("convw", case), make)


def conv_input(case, vol):
    def make():
        b, *dims = CONV_VOLUMES[vol]
        return torch.randn(b, CONV_CASES[case][0], *dims, generator=_gen(4500 + sum(dims) + CONV_CASES[case][0]))
    return _once(("convx", case, vol), make)


def nc_weights(case):
    c = NC_CASES[case]
    return _once(("ncw", case), lambda: synthetic.make_ncn_state_dict(4600 + len(c["channels"]), c["kernel_sizes"], c["channels"], gain=2.0,
                                                                      bias=0.02, prefix=""))


def nc_input():
    def make():
        fa, fb = nr.features(4700, NC_SHAPE)
        fa = fa / (fa.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
        fb = fb / (fb.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
        return nr.mutual_matching(torch.einsum("bcij,bckl->bijkl", fa, fb)).contiguous()
    return _once("ncx", make)


def match_inputs(ksize):
    """(volume [B,1,6,8,4,10], the four int64 relocalisation tensors or None)."""
    def make():
        g = _gen(4800 + ksize)
        x = torch.randn((MATCH_SHAPE[0], 1) + MATCH_SHAPE[1:], generator=g)
        delta = None if ksize == 1 else tuple(torch.randint(0, ksize, x.shape, generator=g) for _ in range(4))
        return x, delta
    return _once(("match", ksize), make)


def pool_nan_case(k=2):
    """(x with NaNs sown into the k = 2 input, pooled, code) by the reference's rule: torch.max over the slices gives NaN and the
    index of the FIRST NaN for a window that holds one (first maximum otherwise)."""
    def make():
        x = pool_input(k).clone()
        idx = torch.randperm(x.numel(), generator=_gen(4250))[:x.numel() // 6]
        x.view(-1)[idx] = float("nan")
        stack = torch.stack([x[:, i::k, j::k, a::k, b::k] for i in range(k) for j in range(k) for a in range(k) for b in range(k)], 1)
        pooled, code = torch.max(stack, dim=1)
        assert pooled.isnan().any() and not pooled.isnan().all()
        nan_first = stack.isnan().to(torch.int64).argmax(dim=1)
        assert torch.equal(code[pooled.isnan()], nan_first[pooled.isnan()])
        return x, pooled, code
    return _once(("poolnan", k), make)


def input_digest(*tensors):
    """sha256 over the bytes of seeded inputs: a fixture that stores outputs only records it, so that another random stream is
    reported as such and not as a numerical failure."""
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def l2_input(case):
    shape, _ = L2_CASES[case]
    return _once(("l2", case), lambda: torch.randn(shape, generator=_gen(4900 + len(shape) + shape[0])))


# ---- float64 restatements ------------------------------------------------------------------------------------------------------
def l2_normalize64(x, dim):
    """modules.py:6."""
    x = x.double()
    return x / torch.pow(torch.sum(torch.pow(x, 2), dim=dim) + 1e-6, 0.5).unsqueeze(dim)


def correlation64(fa, fb):
    """modules.py:41-48 -> [b, h1*w1, h2*w2]."""
    b, c = fa.shape[:2]
    return torch.bmm(fa.double().reshape(b, c, -1).transpose(1, 2), fb.double().reshape(b, c, -1))


def maxpool4d_restated(x, k):
    """modules.py:11-34 on [B,H1,W1,H2,W2] -> (pooled, code s = ((i k + j) k + k') k + l of the first maximum)."""
    slices = [x[:, i::k, j::k, kk::k, l::k] for i in range(k) for j in range(k) for kk in range(k) for l in range(k)]
    stack = torch.stack(slices, 1)
    pooled = stack.max(dim=1).values
    first = (stack == pooled.unsqueeze(1)).to(torch.int64).argmax(dim=1)      # argmax of a 0/1 tensor: the first 1
    return pooled, first


def mutual_matching64(x):
    """ncn/model.py:157-176 on [B,hA,wA,hB,wB]."""
    return nr.mutual_matching(x.double())


def conv4d64(x, w_stored, bias):
    """conv4d.py:12-74."""
    return nr.conv4d(x.double(), w_stored.double(), bias.double() if bias is not None else None)


def neigh_consensus64(x, case):
    """ncn/model.py:145-155 on [B,hA,wA,hB,wB]."""
    return nr.restate(x, nc_weights(case), NC_CASES[case])


def rel_err(out, ref64):
    scale = ref64.abs().max().item()
    return (out.double() - ref64).abs().max().item() / scale


def check_measured(out, ref64, key, label):
    """max |out - f64| / max |f64| against BAR x REF_ERR[key]; prints the figure before it asserts."""
    err, tol = rel_err(out, ref64), BAR * REF_ERR[key]
    print(f"{key} {label}: relative error {err:.3g}, bar {tol:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"{key} {label}: {err:.3g} > {tol:.3g}"


def check_mutual(out, x, label):
    ref = mutual_matching64(x)
    nz = ref != 0
    err = ((out.double() - ref).abs()[nz] / ref.abs()[nz]).max().item()
    print(f"mutual matching {label}: relative error {err:.3g}, bar {MM_BAR:.3g}")
    assert err <= MM_BAR and (out[~nz] == 0).all()


def check_l2(out, x, dim, label):
    ref = l2_normalize64(x, dim)
    nz = ref != 0
    err = ((out.double() - ref).abs()[nz] / ref.abs()[nz]).max().item()
    print(f"L2Normalize {label}: relative error {err:.3g}, bar {l2_bar(x.shape[dim]):.3g}")
    assert err <= l2_bar(x.shape[dim])


# every direction / option of the extractors: (name, ksize, kwargs)
def match_cases():
    out = []
    for inv in (False, True):
        for ksize in (1, 2):
            for soft in (True, False):
                out.append((f"m_inv{int(inv)}_k{ksize}_s{int(soft)}", ksize,
                            dict(ksize=ksize, do_softmax=soft, invert_matching_direction=inv)))
    return out


def coord_cases():
    return [(f"c_inv{int(inv)}_k{ksize}_{scale}", ksize, dict(ksize=ksize, do_softmax=False, scale=scale, invert_matching_direction=inv,
                                                              return_indices=False))
            for inv in (False, True) for ksize in (1, 2) for scale in ("positive", "centered")]


def topk_cases():
    return [(f"t_inv{int(inv)}_k{ksize}_s{int(soft)}_top{topk}", ksize,
             dict(topk=topk, ksize=ksize, do_softmax=soft, invert_matching_direction=inv))
            for inv in (False, True) for ksize in (1, 2) for soft in (True, False) for topk in (1, 3)]
