"""Coarse mode 'fp16' (P2P_COARSE_FP16: one fp16 plane per operand, one MFMA per product in prep_kernel, corr_pool_kernel and
nc_fused_kernel) -- the case table, the seeded inputs, the fp64 yardstick, the error bounds and the runner shared by
tests/test_coarse_mode_host.py, tests/test_coarse_mode_emulated.py (the kernels' code on the CPU, tests/hipemu) and
tests/test_gpu_coarse_mode.py (MI355X).

YARDSTICK.  oracle/p2p_oracle.py's coarse stage in fp64 on the fp32 inputs (`Yardstick`: the stages of `coarse_forward`, kept
apart so that every intermediate volume has its own bound).

BOUNDS, per element.  u = 2^-24 (fp32); eps = 2^-11 in mode 'fp16', 2^-24 in the default mode (the figure the sources state for
the two-plane split); NPROD = MFMA products per fp32 product (1 / 3).
  operand      Every operand is rounded once to fp16 behind an exact power-of-two scale s: d(x) <= max(eps |x s|, 2^-24) / s for
               x != 0 and 0 for x = 0 (`operand_error`; the floor is the subnormal spacing of fp16, absolute).
  normalise    n = f / sqrt(sum f^2 + 1e-6) in fp32: the sum of C squares (<= (C + 2) u relative), halved by the root, the
               root, the division and the product: <= ENORM = (0.5 (C + 2) + 4) u relative to |n|.
  correlation  operands |n| + dn with dn = ENORM |n| + d(|n| (1 + ENORM)), s = 2^12:
               |dc| <= corr(|na| + dna, |nb| + dnb) - corr(|na|, |nb|) + NPROD K u corr(|na| + dna, |nb| + dnb)
               (= (2 eps + eps^2) sum |a||b| + K u sum |a||b| + the normalisation's terms in the normal range); the products of
               fp16 numbers are exact in fp32, the un-scaling is a power of two.
  max-pool     1-Lipschitz: the bound of a pooled cell is the largest bound in its window.  A relocalisation code may differ
               from the fp64 one only where the fp64 gap of the two candidates is within the sum of their bounds.
  mutual m.    x = p^3 / (R C), R = r + 1e-5, C = c + 1e-5 (r, c: the row / column maxima, 1-Lipschitz in p: er, ec = the largest
               input bound of the row / column).  oracle/error_model.py:_mm_err is the first-order form of this (3 p^2 ep / (R C));
               with eps = 2^-11 the input bound ep is not small against a small p, so `mm_bound` keeps every order:
               |dx| <= ((|p| + ep)^3 - |p|^3) / ((R - er)(C - ec)) + |x| (R ec + C er + er ec) / ((R - er)(C - ec)) + 6 u |x|
               (infinite where a maximum is not known to be positive: such a cell asserts nothing).
  consensus    per branch, X under s = 2^12 2^-E (E from max |X| as the kernel takes it; the floor is doubled for a maximum at a
               power of two), the weights of layer 1 per channel and of layer 2 per branch to the top of [2^11, 2^12), the
               hidden volume under 2^sh 2^-E (pack_nc_fused):
               e1 = conv(|x| + e_in + dx, |W1| + dW1) - conv(|x|, |W1|) + NPROD K1 u conv(|x| + e_in + dx, |W1| + dW1)
                    + 3 u (|W1| * |x| + |b1|)                       K1 = 81; bias, scale and fma in fp32
               ReLU is 1-Lipschitz; the hidden value is rounded once more: dh = d(|h| + e1)
               e2 = conv(|h| + e1 + dh, |W2| + dW2) - conv(|h|, |W2|) + (NPROD K2 + 12) u conv(|h| + e1 + dh, |W2| + dW2)
                    + 3 u (|W2| * |h| + |b2|)                       K2 = 16 x 81; nine fp32 additions into the tile's accumulators
               The branches add (one fp32 addition: u |y|).  Evaluated with orc.conv4d on absolute values.
  second m.m.  as the first.
The tests assert these bounds, never a measured value; measured / bound is printed per stage.

CASES.  The smallest shapes at which the kernels can still go wrong (see CASES below).  FEATURES are "planted": the B cells are
a seeded selection of the A cells plus noise, so winners have real margins; `Yardstick.decidable` marks the rows whose fp64
winner beats the runner-up by more than the sum of the two bounds, and `assert_decidable_share` requires at least half of all
rows of every case to be decidable under the 'fp16' bound -- later changes of the inputs cannot hollow the index assertions
out.  The consensus weights are the seeded synthetic checkpoint (golden_util.state_dict(0), utils/synthetic.py: scaled there
for plentiful mutual matches); no further scaling was needed."""
import ctypes

import torch

from oracle import p2p_oracle as orc

U32 = 2.0 ** -24
EPS = {"fp16": 2.0 ** -11, "fp16x2": 2.0 ** -24}
NPROD = {"fp16": 1, "fp16x2": 3}
MODE_IDS = {"fp16x2": 0, "fp16": 1}                    # P2P_COARSE_FP16X2 / P2P_COARSE_FP16 (include/p2p_hip.h)
FLOOR = 2.0 ** -24

# name -> (C, (hA, wA), (hB, wB), ksize, pairs, gpu_only)
CASES = {
    "c32_6x8_k1": (32, (6, 8), (6, 8), 1, 1, False),
    "c64_12x16_k2": (64, (12, 16), (12, 16), 2, 1, False),
    "c32_12x16_k1_tiles": (32, (12, 16), (12, 16), 1, 1, False),     # 192 x 192 cells: 2 x 2 GEMM tiles, consensus tiles along b and c,
                                                                     # several strips, ring restaging, partial tiles
    "c32_8x12_12x8_k2": (32, (8, 12), (12, 8), 2, 1, False),         # B image of another size
    "c256_6x8_k1": (256, (6, 8), (6, 8), 1, 1, False),               # the full K loop of the correlation
    "c32_8x8_k2_batch3": (32, (8, 8), (8, 8), 2, 3, False),          # magnitudes 1, 2^10, 2^-10; pair 1 has dead cells
    "c32_24x32_k4": (32, (24, 32), (24, 32), 4, 1, True),            # MI355X only: 768 x 768 GEMM rows in the emulator are slow
}
EMU_CASES = [k for k, v in CASES.items() if not v[5]]
ALL_CASES = list(CASES)


def case_inputs(name):
    """Seeded (fa [B,C,hA,wA], fb [B,C,hB,wB]) fp32 of a case: planted pairs (module docstring)."""
    c, (ha, wa), (hb, wb), k, pairs, _ = CASES[name]
    gen = torch.Generator().manual_seed(4000 + 17 * list(CASES).index(name))
    fa = torch.randn(pairs, c, ha * wa, generator=gen)
    fb = torch.empty(pairs, c, hb * wb)
    # the planting is per pooling cell (a cell of B is a cell of A with its k x k positions shuffled): the pooled volume then has
    # one strong candidate per row, as a fine-level permutation has for k = 1
    nac, nbc, wac, wbc = (ha // k) * (wa // k), (hb // k) * (wb // k), wa // k, wb // k
    for z in range(pairs):
        cell = torch.cat([torch.randperm(nac, generator=gen) for _ in range((nbc + nac - 1) // nac)])[:nbc]
        src = torch.empty(hb * wb, dtype=torch.long)
        for cb in range(nbc):
            ca, sub = int(cell[cb]), torch.randperm(k * k, generator=gen)
            for q in range(k * k):
                qa = int(sub[q])
                pb = ((cb // wbc) * k + q // k) * wb + (cb % wbc) * k + q % k
                src[pb] = ((ca // wac) * k + qa // k) * wa + (ca % wac) * k + qa % k
        fb[z] = fa[z][:, src] + 0.3 * torch.randn(c, hb * wb, generator=gen)
    if pairs == 3:
        mag = torch.tensor([1.0, 1024.0, 1.0 / 1024.0]).view(3, 1, 1)
        fa, fb = fa * mag, fb * mag
        fa.view(pairs, c, ha, wa)[1, :, 2:4, 2:6] = 0.0    # a block of exact zeros: two dead pooling cells
    return fa.view(pairs, c, ha, wa).contiguous(), fb.view(pairs, c, hb, wb).contiguous()


# ---- bounds (fp64) ---------------------------------------------------------------------------------------------------------
def operand_error(t_abs, scale, eps, floor=FLOOR):
    """Bound on |t^ - t| for operands of magnitude t_abs (fp64) rounded once to fp16 under the power-of-two `scale`."""
    ts = t_abs * scale
    d = torch.maximum(eps * ts, torch.full_like(ts, floor))
    return torch.where(ts == 0, torch.zeros_like(ts), d) / scale


def pow2_to_top(mx, target=12):
    """The exact power of two s with mx s in [2^(target-1), 2^target) (1 for mx = 0): host_pack.h's pow2_exponent_to."""
    _, e = torch.frexp(mx)
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), target - e), torch.ones_like(mx))


def corr_bound(na_abs, nb_abs, mode, enorm=None):
    """|kernel correlation - exact| per cell for normalised features of magnitude na_abs [C,h,w], nb_abs (fp64)."""
    c = na_abs.shape[0]
    enorm = (0.5 * (c + 2) + 4) * U32 if enorm is None else enorm
    da = enorm * na_abs + operand_error(na_abs * (1 + enorm), 4096.0, EPS[mode])
    db = enorm * nb_abs + operand_error(nb_abs * (1 + enorm), 4096.0, EPS[mode])
    full = orc.correlation(na_abs + da, nb_abs + db)
    return full - orc.correlation(na_abs, nb_abs) + NPROD[mode] * c * U32 * full


def mm_bound(p, ep):
    """MutualMatching (ncn/model.py:157-176) of the fp64 volume p known to ep -> (x, bound); module docstring."""
    r = p.amax(dim=(2, 3), keepdim=True) + 1e-5
    c = p.amax(dim=(0, 1), keepdim=True) + 1e-5
    er = ep.amax(dim=(2, 3), keepdim=True)
    ec = ep.amax(dim=(0, 1), keepdim=True)
    x = p * ((p / r) * (p / c))
    den = (r - er) * (c - ec)
    ok = ((r - er) > 0) & ((c - ec) > 0)
    den = torch.where(ok, den, torch.ones_like(den))
    pa = p.abs()
    ex = ((pa + ep) ** 3 - pa ** 3) / den + x.abs() * (r * ec + c * er + er * ec) / den + 6 * U32 * x.abs()
    return x, torch.where(ok.expand_as(ex), ex, torch.full_like(ex, float("inf")))


def conv_bound(x_abs, e_in, w, b, w_scale, x_scale, mode, k_terms, extra_u=0, floor=FLOOR):
    """One consensus layer: bound on |kernel(x~) - exact(x)| before the ReLU for inputs |x| (fp64 [ci,...]) known to e_in and
    rounded under x_scale, stored weights w under w_scale (broadcastable to w)."""
    w_abs = w.abs()
    zb = torch.zeros_like(b)
    dx = operand_error(x_abs + e_in, x_scale, EPS[mode], floor)
    dw = operand_error(w_abs, w_scale, EPS[mode])
    s = orc.conv4d(x_abs, w_abs, zb)
    full = orc.conv4d(x_abs + e_in + dx, w_abs + dw, zb)
    return full - s + (NPROD[mode] * k_terms + extra_u) * U32 * full + 3 * U32 * (s + b.abs().view(-1, 1, 1, 1, 1))


def branch_scales(ncn, transposed):
    """The power-of-two scales pack_nc_fused gives one branch: (layer-1 weights per channel [1,16,1,1,1,1] in the stored layout,
    hidden volume, layer-2 weights)."""
    w1, b1, w2 = ncn["w1"], ncn["b1"], ncn["w2"]           # stored layouts [3,16,1,3,3,3], [3,1,16,3,3,3]: both branches hold
    s1 = pow2_to_top(w1.abs().amax(dim=(0, 2, 3, 4, 5), keepdim=True))       # the same numbers, so the maxima are the same
    hmax = (w1.abs().sum(dim=(0, 2, 3, 4, 5)) + b1.abs()).max()
    sh = pow2_to_top(2 * hmax, 13)
    s2 = pow2_to_top(w2.abs().max())
    return s1, sh, s2


def consensus_bound(x, ex, ncn, mode):
    """(y, e_y) of one branch net(x) on the fp64 volume x [a,b,c,d] known to ex."""
    w1, b1, w2, b2 = ncn["w1"], ncn["b1"], ncn["w2"], ncn["b2"]
    s1, sh, s2 = branch_scales(ncn, False)
    amax = float(x.abs().max())
    # the kernel's E: the exponent that brings max |X| below 1; a maximum at a power of two may fall on either side in fp32
    e_x = 0
    while amax / 2.0 ** e_x >= 1.0:
        e_x += 1
    down = 2.0 ** -e_x
    h_pre = orc.conv4d(x[None], w1, b1)
    e1 = conv_bound(x.abs()[None], ex[None], w1, b1, s1, torch.tensor(4096.0 * down, dtype=x.dtype), mode, 81, floor=2 * FLOOR)
    h = h_pre.relu()                                       # 1-Lipschitz: e1 holds for the hidden value too
    y_pre = orc.conv4d(h, w2, b2)
    # the rounding of the hidden volume under 2^sh 2^-E is conv_bound's operand rounding of its input
    e2 = conv_bound(h, e1, w2, b2, torch.full_like(w2, float(s2)), sh * down, mode, 16 * 81, extra_u=12, floor=2 * FLOOR)
    return y_pre.relu()[0], e2[0]


class Yardstick:
    """fp64 stages of one pair (fa [C,hA,wA], fb [C,hB,wB] fp32) with the bound of `mode` per element:
    corr / e_corr (pooled), code (fp64 relocalisation code or None), win / e_win (the k^4 windows and their bounds),
    x / e_x (first mutual matching), y / e_y (consensus, both branches), z / e_z (second mutual matching)."""

    def __init__(self, fa, fb, ksize, sd, mode):
        ncn, _, _ = orc.split_params(sd, torch.float64)
        fa, fb = fa.double(), fb.double()
        na, nb = orc.l2_normalize(fa, 0), orc.l2_normalize(fb, 0)
        c = orc.correlation(na, nb)
        ec = corr_bound(na.abs(), nb.abs(), mode)
        self.ksize, self.mode = ksize, mode
        self.code = self.win = self.e_win = None
        if ksize > 1:
            k = ksize
            ha, wa, hb, wb = c.shape
            win = lambda t: t.reshape(ha // k, k, wa // k, k, hb // k, k, wb // k, k).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(
                ha // k, wa // k, hb // k, wb // k, k ** 4)
            self.win, self.e_win = win(c), win(ec)
            c, ec = self.win.amax(-1), self.e_win.amax(-1)
            self.code = self.win.argmax(-1)
        self.corr, self.e_corr = c, ec
        self.x, self.e_x = mm_bound(c, ec)
        y1, e1 = consensus_bound(self.x, self.e_x, ncn, mode)
        t = lambda v: v.permute(2, 3, 0, 1).contiguous()
        y2, e2 = consensus_bound(t(self.x), t(self.e_x), ncn, mode)
        self.y = y1 + t(y2)
        self.e_y = e1 + t(e2) + U32 * self.y.abs()
        self.z, self.e_z = mm_bound(self.y, self.e_y)

    def decidable(self):
        """(winner, decidable?) for the nB rows B->A followed by the nA rows A->B (the order of cal_coarse_matches): the fp64
        winner's lower end lies above every competitor's upper end."""
        ha, wa, hb, wb = self.z.shape
        m, e = self.z.reshape(ha * wa, hb * wb), self.e_z.reshape(ha * wa, hb * wb)
        out = []
        for dim in (0, 1):
            best = m.argmax(dim=dim)
            hi2 = (m + e).clone()
            if dim == 0:
                cols = torch.arange(hb * wb)
                lo = (m - e)[best, cols]
                hi2[best, cols] = -float("inf")
            else:
                rows = torch.arange(ha * wa)
                lo = (m - e)[rows, best]
                hi2[rows, best] = -float("inf")
            out.append((best, lo > hi2.amax(dim=dim)))
        return torch.cat((out[0][0], out[1][0])), torch.cat((out[0][1], out[1][1]))


_yard_cache = {}


def yardsticks(name, sd, mode):
    """One Yardstick per pair of a case (computed once per process and mode; never modified)."""
    key = (name, mode)
    if key not in _yard_cache:
        fa, fb = case_inputs(name)
        _yard_cache[key] = [Yardstick(fa[z], fb[z], CASES[name][3], sd, mode) for z in range(fa.shape[0])]
    return _yard_cache[key]


def assert_decidable_share(name, sd):
    """At least half of all coarse rows of the case are decidable under the 'fp16' bound -> the share."""
    dec = torch.cat([y.decidable()[1] for y in yardsticks(name, sd, "fp16")])
    share = float(dec.double().mean())
    assert share >= 0.5, f"{name}: only {share:.2f} of the coarse rows are decidable under the fp16 bound"
    return share


# ---- runner: the C ABI on CPU tensors (emulated library) or device tensors (the real one) --------------------------------------
def bind(lib):
    """Prototypes of the two symbols of the mode (tests/hipemu/emu_lib.py copies the ones patch2pix_amd/_lib.py lists; this keeps
    the emulated module usable with an older list)."""
    lib.p2p_ncn_set_mode.argtypes, lib.p2p_ncn_set_mode.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    lib.p2p_ncn_get_mode.argtypes, lib.p2p_ncn_get_mode.restype = [ctypes.c_void_p], ctypes.c_int
    return lib


def _al(b):
    return (b + 255) & ~255


def workspace_layout(c, ha, wa, hb, wb, k):
    """Byte offsets of a pair's block of the coarse workspace (csrc/coarse_api.hip:coarse_ws, tuned handles)."""
    na, nb = ha * wa, hb * wb
    nac, nbc = na // (k * k), nb // (k * k)
    off, lay = 0, {}
    for key, size in (("fnA", (na + 127) // 128 * 128 * c * 4), ("fnB", (nb + 127) // 128 * 128 * c * 4), ("P", nac * nbc * 4),
                      ("Y", nac * nbc * 4), ("Y2", nac * nbc * 4), ("keys", (2 * (nac + nbc) + 1) * 4)):
        lay[key] = off
        off += _al(size)
    lay["total"] = off
    return lay


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


GUARD = 4096


def run_coarse(lib, ncn, fa, fb, ksize, ws_pairs=None, stream=None):
    """p2p_coarse_forward_batch on fa, fb [B,C,h,w] (CPU tensors with the emulated library, device tensors with the real one).
    The workspace and a guard band behind it are pre-filled with 0xFF; the guard band must come back intact.
    -> dict(corr [B,a,b,c,d], delta uint8 or None, x (first mutual matching), y (consensus, both branches added): the last
    two read back from the workspace blocks, for the pairs of the LAST launch only when ws_pairs < B)."""
    fa, fb = fa.contiguous(), fb.contiguous()
    nb_, c, ha, wa = fa.shape
    _, _, hb, wb = fb.shape
    k = max(ksize, 1)
    dev = fa.device
    shape = (nb_, ha // k, wa // k, hb // k, wb // k)
    corr = torch.empty(shape, dtype=torch.float32, device=dev)
    delta = torch.empty(shape, dtype=torch.uint8, device=dev) if ksize > 1 else None
    lay = workspace_layout(c, ha, wa, hb, wb, ksize)
    per_pair = lib.p2p_coarse_workspace_bytes(c, ha, wa, hb, wb, ksize)
    assert per_pair == lay["total"], (per_pair, lay["total"])
    held = ws_pairs or nb_
    ws = torch.full((held * per_pair + 256 + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    shift = (-ws.data_ptr()) % 256
    st = lib.p2p_coarse_forward_batch(_ptr(fa), _ptr(fb), nb_, c, ha, wa, hb, wb, ksize, ncn, _ptr(corr), _ptr(delta),
                                      ctypes.c_void_p(ws.data_ptr() + shift), held * per_pair, stream)
    if st != 0:
        raise RuntimeError(f"p2p_coarse_forward_batch: {lib.p2p_last_error().decode()}")
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert bool((ws[shift + held * per_pair:] == 0xFF).all()), "the guard band behind the workspace was written"
    cells = shape[1] * shape[2] * shape[3] * shape[4]
    xs, ys = [], []
    for z in range(min(held, nb_)):
        blk = ws[shift + z * per_pair: shift + (z + 1) * per_pair]
        f = lambda key: blk[lay[key]: lay[key] + 4 * cells].view(torch.float32).view(shape[1:]).clone()
        xs.append(f("P"))
        ys.append(f("Y") + f("Y2"))
    return dict(corr=corr, delta=delta, x=torch.stack(xs), y=torch.stack(ys))


def run_consensus(lib, ncn, x, stream=None):
    """p2p_neigh_consensus_batch on x [B,a,b,c,d]."""
    x = x.contiguous()
    y = torch.empty_like(x)
    nb_, a, b, c, d = x.shape
    ws = torch.zeros(nb_, dtype=torch.int32, device=x.device)
    st = lib.p2p_neigh_consensus_batch(_ptr(x), nb_, a, b, c, d, ncn, _ptr(y), _ptr(ws), nb_ * 4, stream)
    if st != 0:
        raise RuntimeError(f"p2p_neigh_consensus_batch: {lib.p2p_last_error().decode()}")
    if x.device.type == "cuda":
        torch.cuda.synchronize(x.device)
    return y


def run_matches(lib, corr, delta, ksize, upsample=8, stream=None):
    """p2p_coarse_matches_batch (centre = True) -> (rows [B, nB + nA, 4] int64, scores)."""
    nb_, a, b, c, d = corr.shape
    n = a * b + c * d
    m = torch.empty((nb_, n, 4), dtype=torch.int64, device=corr.device)
    s = torch.empty((nb_, n), dtype=torch.float32, device=corr.device)
    st = lib.p2p_coarse_matches_batch(_ptr(corr), _ptr(delta), nb_, a, b, c, d, ksize, upsample, 1, _ptr(m), _ptr(s), stream)
    if st != 0:
        raise RuntimeError(f"p2p_coarse_matches_batch: {lib.p2p_last_error().decode()}")
    if corr.device.type == "cuda":
        torch.cuda.synchronize(corr.device)
    return m, s


def ncn_create(lib, sd):
    keep = [sd[k].detach().float().contiguous() for k in ("ncn.conv.0.weight", "ncn.conv.0.bias", "ncn.conv.2.weight", "ncn.conv.2.bias")]
    h = ctypes.c_void_p()
    st = lib.p2p_ncn_create(*[t.data_ptr() for t in keep], ctypes.byref(h))
    if st != 0:
        raise RuntimeError(f"p2p_ncn_create: {lib.p2p_last_error().decode()}")
    return h


def set_mode(lib, ncn, mode):
    st = lib.p2p_ncn_set_mode(ncn, MODE_IDS[mode])
    assert st == 0, lib.p2p_last_error().decode()
    assert lib.p2p_ncn_get_mode(ncn) == MODE_IDS[mode]


# ---- assertions shared by the emulated and the MI355X tests --------------------------------------------------------------------
def check_stages(out, name, sd, mode, what=""):
    """Every stage output of `out` (run_coarse) within its bound of `mode`, element-wise; relocalisation codes differ from the
    fp64 ones only inside the bounds.  -> {stage: largest error / bound}."""
    ratios = {}
    for z, yd in enumerate(yardsticks(name, sd, mode)):
        for stage, got, ref, bound in (("mutual1", out["x"][z], yd.x, yd.e_x), ("consensus", out["y"][z], yd.y, yd.e_y),
                                       ("mutual2", out["corr"][z], yd.z, yd.e_z)):
            got = got.detach().cpu().double()
            assert got.shape == ref.shape and torch.isfinite(got).all(), (name, stage)
            err = (got - ref).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
            ratios[stage] = max(ratios.get(stage, 0.0), ratio)
            print(f"{what}{name}[{z}] mode {mode} {stage}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.4f}")
            assert ratio <= 1.0, f"{name}[{z}] mode {mode} {stage}: error {ratio:.3f} of its bound"
        if yd.code is not None:
            code = out["delta"][z].detach().cpu().long()
            diff = code != yd.code
            if bool(diff.any()):
                w, e = yd.win[diff], yd.e_win[diff]
                gi, ri = code[diff][:, None], yd.code[diff][:, None]
                gap = w.gather(1, ri) - w.gather(1, gi)
                assert bool((gap <= e.gather(1, ri) + e.gather(1, gi)).all()), f"{name}[{z}] mode {mode}: a relocalisation code moved outside the bounds"
            print(f"{what}{name}[{z}] mode {mode} relocalisation: {int(diff.sum())} of {diff.numel()} codes differ from fp64, all inside the bounds")
    return ratios


def check_rows(rows, name, sd, mode, upsample=8):
    """rows [B, nB + nA, 4] int64 of cal_coarse_matches (centre = True) on the stage's output: every decidable row names the fp64
    winner's cell; -> (rows that differ from the fp64 winner, decidable rows, all rows)."""
    c, (ha, wa), (hb, wb), k, pairs, _ = CASES[name]
    nbad = ndec = ntot = 0
    for z, yd in enumerate(yardsticks(name, sd, mode)):
        best, dec = yd.decidable()
        a, b, cc, d = yd.z.shape
        nB, nA = cc * d, a * b
        r = rows[z].detach().cpu()
        cell = lambda x, y, w: (y // (upsample * k)) * w + x // (upsample * k)
        got = torch.cat((cell(r[:nB, 0], r[:nB, 1], b), cell(r[nB:, 2], r[nB:, 3], d)))
        # (rows B->A: the A cell is the answer; rows A->B: the B cell)
        differ = got != best
        assert not bool((differ & dec).any()), f"{name}[{z}] mode {mode}: {int((differ & dec).sum())} decidable rows do not name the fp64 winner"
        nbad, ndec, ntot = nbad + int(differ.sum()), ndec + int(dec.sum()), ntot + dec.numel()
    return nbad, ndec, ntot
