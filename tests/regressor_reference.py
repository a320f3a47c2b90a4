"""TEST INFRASTRUCTURE: what the tests of the generic regressor share -- the case table, a torch restatement of a generic
FeatRegressNet forward (reference networks/modules.py:56-112; a few F.conv2d / F.linear calls, any dtype), a fine level
built on oracle.p2p_oracle.gather_patch_feats(feat_idx=...) / parse_regressor_out, and ctypes helpers that drive
p2p_regressor_create_config / p2p_regress_batch of either the real library or the CPU emulator's."""
import ctypes
import hashlib

import torch
import torch.nn.functional as F

from oracle import p2p_oracle as orc
from patch2pix_amd.utils import synthetic

COORD_TOL, SCORE_TOL = 1e-3, 1e-5            # the project's bars (tests/test_gpu_parity.py)
COND_COORD, COND_SCORE = 1e-4, 1e-6          # fp32 restatement vs its own fp64 evaluation: a condition on the inputs

# id -> feat_idx, feat_comb, conv dims / kers / strs, fc_dims, shared, seed of the synthetic checkpoint
CASES = {
    "R": dict(feat_idx=[0, 1, 2, 3], feat_comb="pre", conv_dims=[512, 512], conv_kers=[3, 3], conv_strs=[2, 1],
              fc_dims=[512, 256], shared=False, seed=0),          # the released configuration, forced through the generic path
    "A": dict(feat_idx=[1, 2, 3], feat_comb="pre", conv_dims=[64, 64], conv_kers=[3, 3], conv_strs=[2, 1],
              fc_dims=[64, 32], shared=False, seed=11),           # no level 0, K a multiple of 8
    "B": dict(feat_idx=[0], feat_comb="pre", conv_dims=[32], conv_kers=[3], conv_strs=[2],
              fc_dims=[], shared=False, seed=22),                 # K = 6 per tap (padding path), one conv, Linear(32,5) directly
    "C": dict(feat_idx=[0, 2], feat_comb="post", conv_dims=[128, 48], conv_kers=[3, 3], conv_strs=[2, 1],
              fc_dims=[64], shared=False, seed=13),               # non-contiguous levels, 'post', a dim that is no multiple of 32
    "D": dict(feat_idx=[0, 1, 2, 3], feat_comb="pre", conv_dims=[32, 32, 64], conv_kers=[3, 1, 5], conv_strs=[2, 2, 1],
              fc_dims=[48, 32, 16], shared=False, seed=14),       # 1x1 with padding (8x8 -> 5x5), 5x5 kernel, three FC layers
    "E": dict(feat_idx=[2, 3], feat_comb="post", conv_dims=[1024, 16], conv_kers=[3, 3], conv_strs=[1, 2],
              fc_dims=[1024], shared=True, seed=15),              # widest dims, stride 1 first (16x16 map), shared=True
}
# sha256 over the sorted (key, bytes) of synthetic.make_state_dict(0) with default arguments, recorded from the commit before
# the generator learnt other configurations (a517d01): the default draws must keep their order
DEFAULT_SD_SHA256 = "7fd09d35bb3a9144b4593fc06c39090656d262b33e256627e641c30f6d66e818"


# the inputs of the two kernel tests: name -> (H, W, pyramid seed, proposals); the conditioning test covers exactly these
INPUTS = {"emu": (48, 64, 31, 11), "gpu": (96, 128, 41, 61)}
_inputs = {}


def inputs(name):
    """(pyramid 1, pyramid 2, proposals int64 [n,4]) of a test: "emu" -- 48x64, three hand-picked proposals (the second one's
    windows across two image corners) + 8 random ones; "gpu" -- 96x128, the four corner pairs + 57 random ones."""
    if name not in _inputs:
        h, w, seed, n = INPUTS[name]
        p1, p2 = synthetic.make_pyramid(seed, h, w), synthetic.make_pyramid(seed + 1, h, w)
        if name == "emu":
            fixed = [[20, 24, 30, 20], [2, 3, 61, 45], [40, 10, 8, 40]]
        else:
            fixed = [[0, 0, w - 1, h - 1], [w - 1, 0, 0, h - 1], [0, h - 1, w - 1, 0], [w - 1, h - 1, 0, 0]]
        gen = torch.Generator().manual_seed(seed)
        k = n - len(fixed)
        rnd = torch.stack([torch.randint(0, w, (k,), generator=gen), torch.randint(0, h, (k,), generator=gen),
                           torch.randint(0, w, (k,), generator=gen), torch.randint(0, h, (k,), generator=gen)], dim=1)
        _inputs[name] = (p1, p2, torch.cat([torch.tensor(fixed, dtype=torch.int64), rnd]))
    return _inputs[name]


def sd_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    return h.hexdigest()


def regressor_config(case):
    c = CASES[case]
    return synthetic.default_regressor_config(conv_dims=list(c["conv_dims"]), conv_kers=list(c["conv_kers"]),
                                              conv_strs=list(c["conv_strs"]), fc_dims=list(c["fc_dims"]),
                                              feat_comb=c["feat_comb"], shared=c["shared"])


_ckpt = {}


def checkpoint(case):
    """The seeded synthetic checkpoint of a case, backbone included (built once per process; never modified by a test)."""
    if case not in _ckpt:
        c = CASES[case]
        _ckpt[case] = synthetic.make_checkpoint(c["seed"], regressor_config=regressor_config(case), feat_idx=c["feat_idx"])
    return _ckpt[case]


def sub_params(sd, prefix, dtype=torch.float32):
    return {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix) and v.is_floating_point()}


def case_params(case, dtype=torch.float32):
    sd = checkpoint(case)["state_dict"]
    return sub_params(sd, "regress_mid.", dtype), sub_params(sd, "regress_fine.", dtype)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _bn(x, p, prefix, shape):
    g = lambda k: p[f"{prefix}.{k}"].view(shape)
    return (x - g("running_mean")) / torch.sqrt(g("running_var") + 1e-5) * g("weight") + g("bias")


WINO_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))      # B^T of Winograd F(2x2, 3x3)


def wino_input_transform(h):
    """B^T d B over the sixteen 4 x 4 windows d (stride 2) of the zero-ringed 8 x 8 map h [N,C,8,8], in h's dtype ->
    [N, 16 windows (ty * 4 + tx), 16 positions (i * 4 + j), C]."""
    bt = torch.tensor(WINO_BT, dtype=h.dtype)
    d = F.pad(h, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)          # [N,C,ty,tx,a,b]
    u = torch.einsum("ia,nctxab,jb->ntxijc", bt, d, bt)
    return u.reshape(h.shape[0], 16, 16, h.shape[1])


def regressor_forward(f1, f2, p, case, stages=False):
    """FeatRegressNet.forward (modules.py:101-112) in eval mode, in the dtype of its arguments -> raw [N,5].
    stages (the two-convolution 'pre' configurations with an 8 x 8 map, case "R"): -> (raw, H, U, V) with H = BN1(conv1(x))
    [N,C,8,8] (no ReLU: the network has none there), U = wino_input_transform(H), V = relu(max(BN2(conv2(H)))) [N,C] --
    the values the tuned kernels hand from one launch to the next (tests/stage_reference.py)."""
    c = CASES[case]
    kept = []

    def conv(u):
        for i, st in enumerate(c["conv_strs"]):
            u = _bn(F.conv2d(u, p[f"conv.{2 * i}.weight"], None, stride=st, padding=1), p, f"conv.{2 * i + 1}", (1, -1, 1, 1))
            kept.append(u)
        return F.relu(u).amax(dim=(2, 3))          # one ReLU after the last BatchNorm, MaxPool over the whole map

    v = torch.cat([conv(f1), conv(f2)], dim=1) if c["feat_comb"] == "post" else conv(torch.cat([f1, f2], dim=1))
    pooled = v
    for i in range(len(c["fc_dims"])):
        v = F.relu(_bn(F.linear(v, p[f"fc.{3 * i}.weight"], p[f"fc.{3 * i}.bias"]), p, f"fc.{3 * i + 1}", (1, -1)))
    n = 3 * len(c["fc_dims"])
    raw = F.linear(v, p[f"fc.{n}.weight"], p[f"fc.{n}.bias"])
    if not stages:
        return raw
    assert c["feat_comb"] == "pre" and len(kept) == 2 and kept[0].shape[2:] == (8, 8), "stages: a two-convolution 'pre' net on an 8 x 8 map"
    return raw, kept[0], wino_input_transform(kept[0]), pooled


def fine_level(pyr1, pyr2, matches, p, case):
    """forward_fine_match of one batch item (patch2pix.py:157-218) -> (matches [N,4], probs [N], raw [N,5])."""
    fi = tuple(CASES[case]["feat_idx"])
    h1, w1 = pyr1[0].shape[1:]
    h2, w2 = pyr2[0].shape[1:]
    mi = matches.long()                              # networks/utils.py:19 (trunc)
    f1 = orc.gather_patch_feats(pyr1[:4], mi[:, 0], mi[:, 1], feat_idx=fi)
    f2 = orc.gather_patch_feats(pyr2[:4], mi[:, 2], mi[:, 3], feat_idx=fi)
    out = regressor_forward(f1, f2, p, case)
    return orc.parse_regressor_out(out, matches, w1, h1, w2, h2) + (out,)


def to_dtype(pyr, dtype):
    return [t.to(dtype) for t in pyr]


def check_levels(out, pyr1, pyr2, props, case, label=""):
    """The kernel's mid and fine outputs of one pair against the fp32 restatement at the bars; the fine level is fed the kernel's
    own mid matches (so that no proposal has to be excluded for a trunc() flip).  Prints the measured errors."""
    mid_p, fine_p = case_params(case)
    m1, q1, _ = fine_level(pyr1, pyr2, props, mid_p, case)
    errs = [(out["matches1"].cpu() - m1).abs().max().item(), (out["probs1"].cpu() - q1).abs().max().item()]
    if "matches2" in out:
        m2, q2, _ = fine_level(pyr1, pyr2, out["matches1"].cpu(), fine_p, case)
        errs += [(out["matches2"].cpu() - m2).abs().max().item(), (out["probs2"].cpu() - q2).abs().max().item()]
    print(f"case {case} {label}: mid coord {errs[0]:.3g} px score {errs[1]:.3g}" +
          (f", fine coord {errs[2]:.3g} px score {errs[3]:.3g}" if len(errs) > 2 else ""))
    assert errs[0] <= COORD_TOL and errs[1] <= SCORE_TOL, errs
    if len(errs) > 2:
        assert errs[2] <= COORD_TOL and errs[3] <= SCORE_TOL, errs
    return errs


# ---- ctypes: the C ABI of the real library or of the emulator's ------------------------------------------------------------
def fill_config(lay):
    """(p2p_regressor_config, p2p_regressor_tensors) skeleton of a layout dict (CASES entry or ops.regressor_layout)."""
    from patch2pix_amd import _lib as real
    c = real.RegressorConfig()
    c.n_feat = len(lay["feat_idx"])
    for i, j in enumerate(lay["feat_idx"]):
        c.feat_idx[i] = j
    c.feat_comb = real.FEAT_COMB[lay["feat_comb"]]
    c.n_conv, c.n_fc, c.psize = len(lay["conv_dims"]), len(lay["fc_dims"]), 16
    for i in range(c.n_conv):
        c.conv_dim[i], c.conv_ker[i], c.conv_str[i] = lay["conv_dims"][i], lay["conv_kers"][i], lay["conv_strs"][i]
    for i in range(c.n_fc):
        c.fc_dim[i] = lay["fc_dims"][i]
    return c


def create_config(lib, sub_sd, lay):
    """p2p_regressor_create_config on host tensors -> (status, handle); works for the emulator's library too."""
    from patch2pix_amd import _lib as real
    keep = {k: v.detach().float().contiguous() for k, v in sub_sd.items() if v.is_floating_point()}
    bn = lambda pre: real.BnParams(*[keep[f"{pre}.{k}"].data_ptr() for k in ("weight", "bias", "running_mean", "running_var")])
    c, t = fill_config(lay), real.RegressorTensors()
    for i in range(c.n_conv):
        t.conv_w[i] = keep[f"conv.{2 * i}.weight"].data_ptr()
        t.conv_bn[i] = bn(f"conv.{2 * i + 1}")
    for i in range(c.n_fc):
        t.fc_w[i], t.fc_b[i] = keep[f"fc.{3 * i}.weight"].data_ptr(), keep[f"fc.{3 * i}.bias"].data_ptr()
        t.fc_bn[i] = bn(f"fc.{3 * i + 1}")
    t.out_w, t.out_b = keep[f"fc.{3 * c.n_fc}.weight"].data_ptr(), keep[f"fc.{3 * c.n_fc}.bias"].data_ptr()
    h = ctypes.c_void_p()
    st = lib.p2p_regressor_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(h))
    return st, h


def emu_regress(emu, reg1, reg2, pyr1, pyr2, proposals, ws_bytes=None):
    """One pair through the emulator's p2p_regress_batch with a workspace of ws_bytes (None: what
    p2p_regress_workspace_bytes_for asks for) -> dict matches1/probs1/raw1 (+ *2 with reg2)."""
    from patch2pix_amd import _lib as real

    def pyramid(levels):
        lv = [t.contiguous() for t in levels[:4]]
        q = real.Pyramid()
        for j in range(4):
            q.level[j] = lv[j].data_ptr()
        q.height, q.width = lv[0].shape[-2:]
        return q, lv
    pa, ka = pyramid(pyr1)
    pb, kb = pyramid(pyr2)
    n = proposals.shape[0]
    proposals = proposals.contiguous()
    two = reg2 is not None
    out = {k: torch.full((n, c) if c > 1 else (n,), float("nan"), dtype=torch.float32)
           for k, c in (("matches1", 4), ("probs1", 1), ("raw1", 5)) + ((("matches2", 4), ("probs2", 1), ("raw2", 5)) if two else ())}
    need = emu.p2p_regress_workspace_bytes_for(reg1, n) if ws_bytes is None else ws_bytes
    ws = torch.empty(need + 128, dtype=torch.uint8)
    wsp = ctypes.c_void_p((ws.data_ptr() + 127) & ~127)
    g = lambda k: out[k].data_ptr() if k in out else None
    st = emu.p2p_regress_batch(reg1, reg2 if two else None, 1, (real.Pyramid * 1)(pa), (real.Pyramid * 1)(pb),
                               (ctypes.c_int * 1)(n), proposals.data_ptr(), int(proposals.is_floating_point()),
                               g("matches1"), g("probs1"), g("raw1"), g("matches2"), g("probs2"), g("raw2"), wsp, need, None)
    del ka, kb
    assert st == 0, f"p2p_regress_batch returned {st}: {emu.p2p_last_error().decode()}"
    return out
