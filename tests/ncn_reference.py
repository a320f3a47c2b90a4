"""TEST INFRASTRUCTURE: the cases, inputs, torch restatement and tolerances shared by the tests of the generic consensus net
(csrc/consensus_generic.hip): tests/test_ncn_configs_host.py, test_ncn_generic_emulated.py, test_gpu_ncn_configs.py, and the
fixture generator tests/make_golden_ncn.py.

Yardstick: `restate(..., dtype=torch.float64)`, NeighConsensus.forward (reference networks/ncn/model.py:145-155) restated per
layer the way conv4d.py:12-74 computes it -- zero padding, k F.conv3d slices summed, centre slice (with the bias) first,
then the slices p below / p above for p = 1..k//2 -- followed by ReLU after every layer.

Tolerance: REF_ERR[case] is the unmodified reference's own fp32 error against that yardstick, max |ref32 - f64| / max |f64|,
the largest over the three volumes, measured by tests/make_golden_ncn.py (which prints the table below).  The kernel's bar
against fp64 is 4 x REF_ERR (it sums up to 625 x 16 terms in another order than the host convolution library: the bound must
not depend on which order happens to be luckier), against the golden (reference fp32) 5 x REF_ERR.  Bars are relative to the
largest fp64 value of the volume at hand.  Nothing here is derived from the kernel's output.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from patch2pix_amd.utils import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    "R": dict(kernel_sizes=[3, 3], channels=[16, 1], symmetric_mode=True),          # the released shape, built with generic=True
    "N": dict(kernel_sizes=[3, 3, 3], channels=[10, 10, 1], symmetric_mode=True),   # the class's own default
    "P": dict(kernel_sizes=[5, 5, 5], channels=[16, 16, 1], symmetric_mode=True),   # NCNet's PF-Pascal stack
    "M": dict(kernel_sizes=[5, 3], channels=[7, 1], symmetric_mode=False),          # odd channels, mixed kernels, one branch
    "S": dict(kernel_sizes=[3], channels=[1], symmetric_mode=True),                 # single layer
}
# [B, hA, wA, hB, wB]: four distinct sides (a swapped axis shows; side 5 = the 5-tap kernel, every cell touches padding);
# sides below the kernel; one cell
VOLUMES = {"big": (3, 6, 7, 5, 8), "thin": (2, 2, 3, 9, 4), "one": (1, 1, 1, 1, 1)}
# seeds picked on the CPU from the fp64 restatement alone: between a quarter and 85 % of the cells of "big" and "thin" survive
# the last ReLU, and (all but S) the single cell of "one" does
SEEDS = {"R": 121, "N": 112, "P": 153, "M": 124, "S": 105}
# Xavier bounds shrink with the fan (a 5^4 x 16 layer draws from +-0.017): the gains keep the activations of the last layer
# at the magnitude of the input, so that its ReLU passes a substantial share of the cells (MIN_SHARE, asserted below)
GAINS = {"R": 2.0, "N": 2.0, "P": 2.0, "M": 2.0, "S": 2.0}
MIN_SHARE = 0.25

# max |reference fp32 - fp64| / max |fp64| per case (tests/make_golden_ncn.py, the largest of the three volumes)
REF_ERR = {"R": 5.06e-07, "N": 3.68e-07, "P": 1.41e-06, "M": 3.77e-07, "S": 1.29e-07}
BAR_F64, BAR_GOLDEN = 4.0, 5.0


def golden_name(case):
    return os.path.join(HERE, "golden", f"ncn_{case}.npz")


def weights(case):
    """Sub-state_dict of the case's consensus net ('conv.0.weight', ... in the stored layout), fp32."""
    c = CASES[case]
    return synthetic.make_ncn_state_dict(SEEDS[case], c["kernel_sizes"], c["channels"], gain=GAINS[case], bias=0.02, prefix="")


def mutual_matching(x):
    """networks/ncn/model.py:157-176 on [B,hA,wA,hB,wB]."""
    eps = 1e-5
    xa = x / (x.amax(dim=(3, 4), keepdim=True) + eps)
    xb = x / (x.amax(dim=(1, 2), keepdim=True) + eps)
    return x * (xa * xb)


def features(seed, shape, channels=16, shift=0.3):
    """Two batches of post-ReLU-like feature maps [B,C,h,w] for a volume shape; `shift` sets how many channels a cell has
    active (0.3: most of them; -1.0: about one in six, the sparse features of a trained backbone)."""
    b, ha, wa, hb, wb = shape
    gen = torch.Generator().manual_seed(int(seed))
    fa = torch.relu(torch.randn(b, channels, ha, wa, generator=gen) + shift) + 0.01
    fb = torch.relu(torch.randn(b, channels, hb, wb, generator=gen) + shift) + 0.01
    return fa, fb


def volume(name):
    """The consensus net's input for VOLUMES[name]: mutual-matched correlations of random unit features (the pipeline's
    own magnitudes), fp32 [B,hA,wA,hB,wB]."""
    shape = VOLUMES[name]
    fa, fb = features(7000 + sum(shape), shape)
    fa = fa / (fa.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    fb = fb / (fb.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt()
    corr = torch.einsum("bcij,bckl->bijkl", fa, fb)
    return mutual_matching(corr).contiguous()


def conv4d(x, w_stored, bias):
    """conv4d.py:12-74 with pre-permuted filters: x [B,ci,hA,wA,hB,wB], w_stored [k,co,ci,k,k,k] -> [B,co,hA,wA,hB,wB]."""
    k = w_stored.shape[0]
    pad = k // 2
    b, c, h, w, d, t = x.shape
    data = x.permute(2, 0, 1, 3, 4, 5)
    z = torch.zeros((pad,) + tuple(data.shape[1:]), dtype=x.dtype)
    padded = torch.cat((z, data, z), 0)
    out = []
    for i in range(h):
        o = F.conv3d(padded[i + pad], w_stored[pad], bias=bias, stride=1, padding=pad)
        for p in range(1, pad + 1):
            o = o + F.conv3d(padded[i + pad - p], w_stored[pad - p], bias=None, stride=1, padding=pad)
            o = o + F.conv3d(padded[i + pad + p], w_stored[pad + p], bias=None, stride=1, padding=pad)
        out.append(o)
    return torch.stack(out, 0).permute(1, 2, 0, 3, 4, 5).contiguous()


def restate(x, sd, layout, dtype=torch.float64, branch=None):
    """NeighConsensus.forward on x [B,hA,wA,hB,wB] -> the same shape in `dtype`.  branch='direct' / 'transposed': that
    addend alone."""
    n = len(layout["kernel_sizes"])
    ws = [(sd[f"conv.{2 * i}.weight"].to(dtype), sd[f"conv.{2 * i}.bias"].to(dtype)) for i in range(n)]

    def net(v):
        for w, b in ws:
            v = torch.relu(conv4d(v, w, b))
        return v

    v = x.to(dtype).unsqueeze(1)
    direct = net(v)
    if branch == "direct" or (branch is None and not layout["symmetric_mode"]):
        return direct[:, 0]
    transposed = net(v.permute(0, 1, 4, 5, 2, 3)).permute(0, 1, 4, 5, 2, 3)
    if branch == "transposed":
        return transposed[:, 0]
    return (direct + transposed)[:, 0]


_cache = {}


def expected(case, vol):
    """(x fp32, y fp64) of a case and volume, computed once and shared; callers must not modify them."""
    key = (case, vol)
    if key not in _cache:
        x = volume(vol)
        _cache[key] = (x, restate(x, weights(case), CASES[case]))
    return _cache[key]


def check(out, case, vol, label, bar=BAR_F64):
    """max |out - fp64| against bar x REF_ERR x max |fp64|; prints the figure before it asserts."""
    _, y = expected(case, vol)
    scale = y.abs().max().item()
    err = (out.double() - y).abs().max().item()
    tol = bar * REF_ERR[case] * scale
    print(f"case {case} volume {vol} {label}: max err {err:.3g} (relative {err / scale if scale else 0.0:.3g}), bar {tol:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"case {case} volume {vol} {label}: {err:.3g} > {tol:.3g}"


def share_nonzero(case, vol="big"):
    return float((expected(case, vol)[1] > 0).double().mean())


# the last ReLU must leave a substantial share of the cells alive, or the cases test a field of zeros
for _case in CASES:
    assert share_nonzero(_case) >= MIN_SHARE, (_case, share_nonzero(_case))


# ---- the coarse stage around the consensus net (forward_coarse_match, networks/patch2pix.py:120-136) ---------------------------
# A bar on corr4d = MutualMatching(consensus output y), for deciding which match rows an error within the consensus bar can
# flip: out = y * (y / ma) * (y / mb) with y <= ma, mb (the maxima over B and over A), so |d out| <= 3 |dy| + |d ma| + |d mb|
# <= 5 max |dy|, plus the fp32 rounding of the second mutual matching itself (three multiplications, two divisions: < 4 ulp).
# It is used for the decidability rule alone.  Two handles are compared on corr4d at the plain sum of their consensus bars
# (handles_bar): both are fed the same bits by the same correlation and first mutual-matching kernels, the tuned kernel is
# fp32-equivalent (the same 4 x REF_ERR), and the second mutual matching only shrinks a value (y / ma, y / mb <= 1).
MM_GAIN, MM_ULPS = 5.0, 4 * 2.0 ** -24
# The features of a whole model come through the library's own backbone and fp16x2 correlation, which the project bounds at
# 2e-4 relative on corr4d (tests/test_kernels_emulated.py); that term dominates where a pipeline starts from images.
CORR_RTOL = 2e-4
# feature seeds of the coarse comparisons, picked on the CPU: with them the rows whose top-two gap (fp64) is within twice the
# bar are under UNDECIDED_CAP, and the fp32 restatement of the pipeline disagrees with the fp64 one on no decidable row
# (dense features, shift 0.3, pool to a flat volume at ksize 2: 7 % of its rows are all zeros behind the last ReLU whatever
# the seed; the sparse ones leave none)
COARSE_SEEDS, COARSE_SHIFT = {1: 9101, 2: 9102}, -1.0
# image seed of the NC-only checkpoint test (synthetic.make_image_pair at 64x96, case N, ksize 2), picked the same way on the
# backbone evaluated by PyTorch on the CPU: no row of 48 is undecidable at coarse_bar + CORR_RTOL, the smallest top-two gap is
# 1.4e-2 against a bar of 6.5e-4
NC_IMAGE_SEED = 11
UNDECIDED_CAP = 0.05


def pipeline(fa, fb, ksize, sd, layout, dtype=torch.float64):
    """forward_coarse_match of one pair fa [C,hA,wA] / fb [C,hB,wB] in `dtype` -> (corr4d, consensus output, packed delta)."""
    from oracle import p2p_oracle as po
    a, b = po.l2_normalize(fa.to(dtype), 0), po.l2_normalize(fb.to(dtype), 0)
    corr, delta = po.correlation(a, b), None
    if ksize > 1:
        corr, (di, dj, dk, dl) = po.maxpool4d(corr, ksize)
        delta = ((di * ksize + dj) * ksize + dk) * ksize + dl
    y = restate(po.mutual_matching(corr)[None], sd, layout, dtype)[0]
    return po.mutual_matching(y), y, delta


def coarse_bar(case, y64):
    """Absolute bar on corr4d behind one consensus evaluation of a case, for the decidability rule (see MM_GAIN)."""
    return (MM_GAIN * BAR_F64 * REF_ERR[case] + MM_ULPS) * y64.abs().max().item()


def handles_bar(case, y64):
    """Absolute bar on the difference of two handles' corr4d: the sum of both consensus bars."""
    return 2 * BAR_F64 * REF_ERR[case] * y64.abs().max().item()


def best_cells(corr):
    """Per B cell the best A cell, per A cell the best B cell (first maximum), and the top-two gaps: the rows of
    cal_coarse_matches before relocalisation (softmax is monotone).  corr [hA,wA,hB,wB] -> (idx [nB + nA], gap [nB + nA])."""
    ha, wa, hb, wb = corr.shape
    m = corr.reshape(ha * wa, hb * wb)
    out_i, out_g = [], []
    for mat in (m.t(), m):
        top = torch.topk(mat, min(2, mat.shape[1]), dim=1)
        out_i.append(mat.argmax(dim=1))
        out_g.append(top.values[:, 0] - top.values[:, 1] if mat.shape[1] > 1 else torch.full((mat.shape[0],), float("inf"), dtype=mat.dtype))
    return torch.cat(out_i), torch.cat(out_g)


def decidable(corr64, bar):
    """Rows whose best cell survives an error of `bar` on every value: top-two gap above twice the bar."""
    return best_cells(corr64)[1] > 2 * bar


def load_golden(case):
    return dict(np.load(golden_name(case)))


# ---- the C ABI on a library handle (the emulated library or the real one: same prototypes) -------------------------------------
def create_config(lib, sd, layout):
    """p2p_ncn_create_config on host tensors -> (status, handle)."""
    import ctypes
    from patch2pix_amd import _lib as real
    n = len(layout["kernel_sizes"])
    keep = [(sd[f"conv.{2 * i}.weight"].float().contiguous(), sd[f"conv.{2 * i}.bias"].float().contiguous()) for i in range(n)]
    c, t = real.NcnConfig(), real.NcnTensors()
    c.n_layers, c.symmetric = n, int(layout["symmetric_mode"])
    for i in range(n):
        c.kernel_size[i], c.channels[i] = layout["kernel_sizes"][i], layout["channels"][i]
        t.w[i], t.b[i] = keep[i][0].data_ptr(), keep[i][1].data_ptr()
    h = ctypes.c_void_p()
    st = lib.p2p_ncn_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(h))
    return st, h


def emu_consensus(emu, ncn, x, ws_volumes=None, ws_bytes=None, expect_status=0):
    """p2p_neigh_consensus_batch of the emulated library on a CPU tensor x [B,hA,wA,hB,wB]; `ws_volumes`: the workspace holds
    that many volumes (default: all), or `ws_bytes` bytes."""
    import ctypes
    x = x.contiguous()
    y = torch.full_like(x, float("nan"))
    nb, ha, wa, hb, wb = x.shape
    per = emu.p2p_neigh_consensus_workspace_bytes(ncn, ha, wa, hb, wb)
    nbytes = ws_bytes if ws_bytes is not None else per * (ws_volumes or nb)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8)
    base = (ws.data_ptr() + 255) & ~255
    st = emu.p2p_neigh_consensus_batch(ctypes.c_void_p(x.data_ptr()), nb, ha, wa, hb, wb, ncn, ctypes.c_void_p(y.data_ptr()),
                                       ctypes.c_void_p(base), nbytes, None)
    assert st == expect_status, f"p2p_neigh_consensus_batch returned {st}, expected {expect_status}: {emu.p2p_last_error()}"
    return y
