"""TEST INFRASTRUCTURE: the buffers the tuned kernels hand from one launch to the next, restated independently.

Fine stage (modes fp16x2 / fp16x2w): the caller's workspace holds the pooled features V [level][slot][512] fp32 of both
levels, the un-truncated mid matches, and -- fp16x2w -- the inverse scale `hinv` per proposal of a chunk and the
Winograd-transformed conv2 input U of a chunk as the A operand of wino_gemm_kernel.  Coarse stage: the normalised features
of both images as the operands of corr_pool_kernel.  Both operands are two-plane fp16 in swizzled 16 KiB blocks.

This file holds (1) the layout decoders, written from the header comments of regress_common.h / regress_wino.hip /
coarse.hip (torch ops, so that they run on either device), (2) the fp64 stage references, (3) drivers that call the C ABI
(the real library or the emulator's) on a workspace poisoned with 0xFF plus a guard band, and the assertions
tests/test_stage_buffers_emulated.py and tests/test_gpu_stage_buffers.py share."""
import ctypes

import torch

import regressor_reference as rref
from oracle import p2p_oracle as orc

GUARD = 4096                 # bytes of guard band behind every workspace
POISON = 0xFF                # fp16 0xFFFF and fp32 0xFFFFFFFF are NaNs
MARK = -777.0                # what the output arrays hold before a call

# ---- regress_common.h, restated ---------------------------------------------------------------------------------------
WINO_BLK = 16384             # [plane 2][row 128][32 K] fp16
WINO_CHUNK = 3328


def _up(v, m):
    return (v + m - 1) // m * m


def regress_ws_base_floats(n):
    """V of both levels [2][n][512], padded to 32 floats, then the mid matches [n][4] and 32 floats of slack."""
    return _up(2 * n * 512, 32) + 4 * n + 32


def mid_offset_floats(n):
    return _up(2 * n * 512, 32)


def wino_hinv_offset_floats(n):
    return _up(regress_ws_base_floats(n), 64)


def wino_chunk_rows(n):
    return _up(min(n, WINO_CHUNK), 8)


def wino_u_offset_floats(n):
    return _up(wino_hinv_offset_floats(n) + wino_chunk_rows(n), 64)


def regress_ws_floats(n):
    return wino_u_offset_floats(n) + 16 * (wino_chunk_rows(n) // 8) * 16 * (WINO_BLK // 4)


def regress_ws_bytes(n, mode):
    return 4 * {"fp16x2": regress_ws_base_floats, "fp16x2w": regress_ws_floats}[mode](n)


def wino_chunks(n):
    """[(p0, p1)]: whole units of 256 proposals, at most WINO_CHUNK per chunk, sizes as even as the units allow."""
    units, per = (n + 255) // 256, WINO_CHUNK // 256
    nch = max(1, (units + per - 1) // per)
    base, rem = divmod(units, nch)
    out, u = [], 0
    for c in range(nch):
        u1 = u + base + (1 if c < rem else 0)
        out.append((min(n, u * 256), min(n, u1 * 256)))
        u = u1
    return out


# ---- decoders ---------------------------------------------------------------------------------------------------------
def _unswizzle(blocks):
    """[..., row 128, slot 4, 8] -> [..., row 128, piece 4, 8]: piece q of row r is stored at slot q ^ ((r >> 2) & 3)."""
    dev = blocks.device
    row, piece = torch.arange(128, device=dev), torch.arange(4, device=dev)
    slot = piece[None, :] ^ ((row[:, None] >> 2) & 3)
    return torch.gather(blocks, blocks.dim() - 2, slot[:, :, None].expand(blocks.shape))


def decode_U(ws, n, mblocks, proposals=None):
    """The transformed conv2 input of a chunk of `mblocks` row blocks in a workspace sized for n slots:
    [position 16][row block][K chunk 16][plane 2][row 128][slot 4][8 fp16], row = 16 * (proposal & 7) + 4 * ty + tx,
    channel = 32 * K chunk + 8 * piece + e.  -> (hi, lo) fp16 [rows, 16 positions, 512] with row = 16 * proposal + tile, and
    hinv fp32 [8 * mblocks].  proposals: only these chunk-local proposals (rows 16 * k + tile of the k-th one; hinv [k])."""
    u0 = 4 * wino_u_offset_floats(n)
    assert 8 * mblocks <= wino_chunk_rows(n)
    raw = ws[u0:u0 + 16 * mblocks * 16 * WINO_BLK].view(torch.int16).view(16, mblocks, 16, 2, 128, 4, 8)
    h0 = 4 * wino_hinv_offset_floats(n)
    hinv = ws[h0:h0 + 4 * 8 * mblocks].view(torch.float32)
    if proposals is not None:
        p = torch.as_tensor(proposals, device=ws.device, dtype=torch.int64)
        raw = raw[:, p >> 3]
        hinv = hinv[p]
    v = _unswizzle(raw).permute(1, 4, 0, 3, 2, 5, 6).reshape(raw.shape[1] * 128, 16, 2, 512)     # [block * 128 + row][pos][plane][ch]
    if proposals is not None:
        k = torch.arange(p.numel(), device=ws.device)
        rows = (k[:, None] * 128 + 16 * (p[:, None] & 7) + torch.arange(16, device=ws.device)[None, :]).reshape(-1)
        v = v[rows]
    return v[:, :, 0].contiguous().view(torch.float16), v[:, :, 1].contiguous().view(torch.float16), hinv


def decode_V(ws, n, lvl):
    """Pooled convolution features of level lvl (0, 1): fp32 [n slots, 512]."""
    return ws[4 * lvl * n * 512:4 * (lvl + 1) * n * 512].view(torch.float32).view(n, 512)


def coarse_ws_offsets(C, hA, wA, hB, wB, k):
    """Byte offsets of a pair's block of the coarse workspace (tuned consensus handle): every part 256-byte aligned."""
    nA, nB = hA * wA, hB * wB
    cells = (nA // (k * k)) * (nB // (k * k))
    o, off = {}, 0
    for name, size in (("fnA", _up(nA, 128) * C * 4), ("fnB", _up(nB, 128) * C * 4), ("P", cells * 4), ("Y", cells * 4), ("Y2", cells * 4),
                       ("keys", (2 * (nA // (k * k) + nB // (k * k)) + 1) * 4)):
        o[name] = off
        off += _up(size, 256)
    o["total"] = off
    return o


def plane_row(pos, h, w, k, image):
    """Row of the feature planes that holds position pos = i * w + j (tensor): cell-major, the k^2 positions of a pooling
    cell adjacent; k = 4, image A: inside every 32 rows (two cells e of 16 = (di, dj)) row dj + 8 di + 4 e."""
    i, j = pos // w, pos % w
    pp = ((i // k) * (w // k) + (j // k)) * (k * k) + (i % k) * k + (j % k)
    if k == 4 and image == 0:
        e, di, dj = (pp >> 4) & 1, (pp >> 2) & 3, pp & 3
        pp = (pp // 32) * 32 + dj + 8 * di + 4 * e
    return pp


def decode_planes(ws_pair, C, h, w, k, image, offset):
    """The feature planes of one image of one pair: [block of 128 positions][32-channel chunk][plane 2][row 128][slot 4][8].
    ws_pair: the pair's workspace bytes, offset: coarse_ws_offsets(...)["fnA" / "fnB"].
    -> (hi, lo) fp16 [rows, C]: rows 0 .. h*w-1 are the positions in natural order, the rest the pad rows (in the order
    of the positions h*w .. they would hold)."""
    nblk = _up(h * w, 128) // 128
    raw = ws_pair[offset:offset + nblk * 128 * C * 4].view(torch.int16).view(nblk, C // 32, 2, 128, 4, 8)
    v = _unswizzle(raw).permute(0, 3, 2, 1, 4, 5).reshape(nblk * 128, 2, C)
    dev = ws_pair.device
    live = plane_row(torch.arange(h * w, device=dev), h, w, k, image)
    pad = torch.arange(h * w, nblk * 128, device=dev)
    if k == 4 and image == 0:
        e, di, dj = (pad >> 4) & 1, (pad >> 2) & 3, pad & 3
        pad = (pad // 32) * 32 + dj + 8 * di + 4 * e
    order = torch.cat([live, pad])
    assert torch.equal(torch.sort(order)[0], torch.arange(nblk * 128, device=dev)), "the row order is no permutation"
    v = v[order]
    return v[:, 0].contiguous().view(torch.float16), v[:, 1].contiguous().view(torch.float16)


# ---- fp64 (or any dtype) stage references -------------------------------------------------------------------------------
def fine_stages(pyr1, pyr2, matches, params, dtype):
    """One fine level of the released regressor in `dtype` on the proposals `matches` (truncated as the network does):
    -> (H [n,512,8,8], U [n*16 rows, 16 positions, 512], V [n,512])."""
    d = lambda p: [t.to(dtype) for t in p[:4]]
    prm = {k: v.to(dtype) for k, v in params.items()}
    mi = matches.long()
    with torch.no_grad():
        f1 = orc.gather_patch_feats(d(pyr1), mi[:, 0], mi[:, 1])
        f2 = orc.gather_patch_feats(d(pyr2), mi[:, 2], mi[:, 3])
        _, h, u, v = rref.regressor_forward(f1, f2, prm, "R", stages=True)
    return h, u.reshape(-1, 16, 512), v


def coarse_planes_ref(feat, dtype):
    """F / sqrt(sum F^2 + 1e-6) over the channels of feat [C,h,w] in dtype (modules.py:6) -> [h*w, C]."""
    f = feat.to(dtype)
    return orc.l2_normalize(f, 0).reshape(f.shape[0], -1).t().contiguous()


def e_U(hi, lo, hinv, u_ref):
    """Per proposal: max |(hi + lo) * hinv - U| / max |U| over its 16 x 16 x 512 values -> [n] fp64."""
    n = u_ref.shape[0] // 16
    got = (hi.double() + lo.double()).reshape(n, -1) * hinv.double()[:n, None]
    ref = u_ref.double().reshape(n, -1)
    return (got - ref).abs().amax(1) / ref.abs().amax(1)


def e_V(v, v_ref):
    """Per proposal: max_n |V - V64| / max_n |V64| -> [n] fp64; max |V64| > 0 is asserted, not skipped."""
    ref = v_ref.double()
    top = ref.abs().amax(1)
    assert bool((top > 0).all()), "a proposal whose pooled features are all zero"
    return (v.double() - ref).abs().amax(1) / top


# Ratios r = e(kernel) / e(fp32 restatement on the same inputs), both against fp64, worst proposal of the launch.
# platform -> (mode, metric, level) -> r; level = 0, 1 (fine stage), = ksize for the coarse planes.
# "emu": tests/test_stage_buffers_emulated.py as committed with this table, on the 8-core build container (16 x 24 pair,
# n = 9; "stage[emu]" lines of pytest -s).  "gpu": tests/test_gpu_stage_buffers.py of the same commit on an MI355X
# (64 x 96 pair, n = 41; "stage[gpu]" lines).  The emulator's inputs on the MI355X ("stage[emu inputs on the MI355X]")
# gave U 0.95 / 1.44, V 1.56 / 1.46 (fp16x2w) and V 3.28 / 6.76 (fp16x2): the stand-in's MFMA accumulation is up to 4.5x
# LESS accurate than the hardware's on the same inputs ("Numeric domain of the fp16x2 paths").
R_MEASURED = {
    "emu": {("fp16x2w", "U", 0): 2.035, ("fp16x2w", "U", 1): 1.476, ("fp16x2w", "V", 0): 3.931, ("fp16x2w", "V", 1): 4.160,
            ("fp16x2", "V", 0): 14.825, ("fp16x2", "V", 1): 14.068,
            ("coarse", "F", 1): 2.683, ("coarse", "F", 2): 2.819, ("coarse", "F", 4): 1.434},
    "gpu": {("fp16x2w", "U", 0): 1.179, ("fp16x2w", "U", 1): 1.508, ("fp16x2w", "V", 0): 1.409, ("fp16x2w", "V", 1): 1.612,
            ("fp16x2", "V", 0): 5.723, ("fp16x2", "V", 1): 5.329,
            ("coarse", "F", 1): 2.594, ("coarse", "F", 2): 2.594, ("coarse", "F", 4): 1.421},
}


def bar(platform, mode, metric, level=0):
    """2 x the measured ratio, rounded up to a power of two: what the kernel's error may be of the restatement's."""
    r, b = 2.0 * R_MEASURED[platform][(mode, metric, level)], 1.0
    while b < r:
        b *= 2.0
    while b / 2.0 >= r:
        b /= 2.0
    return b


# ---- drivers ------------------------------------------------------------------------------------------------------------
def poisoned(nbytes, dev, align=256):
    """(keep-alive, view of nbytes + GUARD bytes whose address is a multiple of `align`), everything 0xFF."""
    buf = torch.full((nbytes + GUARD + 2 * align,), POISON, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % align
    return buf, buf[off:off + nbytes + GUARD]


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None


def run_fine(lib, reg1, reg2, pyrs1, pyrs2, props, dev, counts=None, stride=None):
    """p2p_regress_batch (counts None: one pair, props [n,4]) or p2p_regress_batch_dev (counts: int32 per item, every
    item owns `stride` slots of props [items * stride, 4]) on a poisoned workspace of exactly
    p2p_regress_workspace_bytes_for(reg1, slots) bytes + guard.  reg1 / reg2: handles (c_void_p) of `lib`; pyramids and
    proposals are moved to dev.  -> dict ws (uint8 [need]), guard, n (slots), matches1/probs1 (+ matches2/probs2)."""
    from patch2pix_amd import _lib as real          # the structure types of the prototypes (the emulator's library shares them)
    dev = torch.device(dev)
    items = 1 if counts is None else len(counts)
    pa, pb, keep = (real.Pyramid * items)(), (real.Pyramid * items)(), []
    single = counts is None
    for i in range(items):
        for arr, pyr in ((pa, pyrs1 if single else pyrs1[i]), (pb, pyrs2 if single else pyrs2[i])):
            lv = [t.to(dev).contiguous() for t in pyr[:4]]
            keep.append(lv)
            for j in range(4):
                arr[i].level[j] = lv[j].data_ptr()
            arr[i].height, arr[i].width = lv[0].shape[-2:]
    props = props.to(dev).contiguous()
    n = props.shape[0]
    assert single or n == items * stride
    two = reg2 is not None
    out = {k: torch.full((n, 4) if k[0] == "m" else (n,), MARK, dtype=torch.float32, device=dev)
           for k in ("matches1", "probs1") + (("matches2", "probs2") if two else ())}
    need = lib.p2p_regress_workspace_bytes_for(reg1, n)
    keep_ws, ws = poisoned(need, dev)
    g = lambda k: ctypes.c_void_p(out[k].data_ptr()) if k in out else None
    tail = (ctypes.c_void_p(props.data_ptr()), int(props.is_floating_point()), g("matches1"), g("probs1"), None, g("matches2"), g("probs2"), None,
            ctypes.c_void_p(ws.data_ptr()), need, _stream(dev))
    if single:
        st = lib.p2p_regress_batch(reg1, reg2, 1, pa, pb, (ctypes.c_int * 1)(n), *tail)
    else:
        cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        keep.append(cnt)
        st = lib.p2p_regress_batch_dev(reg1, reg2, items, pa, pb, ctypes.c_void_p(cnt.data_ptr()), stride, *tail)
    _sync(dev)
    assert st == 0, f"p2p_regress_batch returned {st}: {lib.p2p_last_error().decode()}"
    del keep
    out.update(ws=ws[:need], guard=ws[need:], n=n, _keep=keep_ws)
    return out


def run_coarse(lib, ncn, fa, fb, ksize, dev):
    """p2p_coarse_forward_batch of fa [B,C,hA,wA] / fb [B,C,hB,wB] on a poisoned workspace of exactly B pairs + guard
    -> dict ws (uint8 [B, per_pair]), guard, corr."""
    dev = torch.device(dev)
    fa, fb = fa.to(dev).contiguous(), fb.to(dev).contiguous()
    nb, c, ha, wa = fa.shape
    hb, wb = fb.shape[2:]
    k = ksize
    shape = (nb, ha // k, wa // k, hb // k, wb // k)
    corr = torch.empty(shape, dtype=torch.float32, device=dev)
    delta = torch.empty(shape, dtype=torch.uint8, device=dev) if k > 1 else None
    per_pair = lib.p2p_coarse_workspace_bytes_for(ncn, c, ha, wa, hb, wb, k)
    keep_ws, ws = poisoned(nb * per_pair, dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lib.p2p_coarse_forward_batch(p(fa), p(fb), nb, c, ha, wa, hb, wb, k, ncn, p(corr), p(delta), p(ws), nb * per_pair, _stream(dev))
    _sync(dev)
    assert st == 0, f"p2p_coarse_forward_batch returned {st}: {lib.p2p_last_error().decode()}"
    return dict(ws=ws[:nb * per_pair].view(nb, per_pair), guard=ws[nb * per_pair:], corr=corr, per_pair=per_pair, _keep=keep_ws)


# ---- shared assertions --------------------------------------------------------------------------------------------------
def guard_intact(res):
    return bool((res["guard"] == POISON).all()) and res["guard"].numel() == GUARD


def _bits(t):
    return t.view(torch.int16)


def is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def is_zero_bits(t):
    return bool((t.contiguous().view(torch.uint8) == 0).all())


def assert_planes_sane(hi, lo, bound, what, strict=True):
    """No NaN / Inf pattern, |hi + lo| < bound (<= when not strict), and the split is canonical: fp16(fp32 hi + fp32 lo) == hi.
    One exception, and no other: lo = fp16(x - hi) may round UP to exactly half a unit of hi's last place (x - hi carries
    more bits than fp16 keeps), and then the sum sits halfway between hi and its neighbour, where rounding to even may pick
    the neighbour.  There the sum must be that exact tie: |s - hi| == |s - fp16(s)|."""
    for name, t in (("hi", hi), ("lo", lo)):
        assert bool(((_bits(t) & 0x7C00) != 0x7C00).all()), f"{what}: an fp16 NaN or Inf pattern in plane {name}"
    s = hi.float() + lo.float()
    top = float(s.abs().max())
    assert top < bound if strict else top <= bound, f"{what}: |hi + lo| reaches {top} (bound {bound})"
    r = s.half()
    off = r != hi
    assert bool(((s - hi.float()).abs() == (s - r.float()).abs())[off].all()), f"{what}: hi is not an fp16 nearest to hi + lo"
    assert int(off.sum()) * 256 <= off.numel(), f"{what}: {int(off.sum())} of {off.numel()} values sit on a rounding tie"


def assert_pow2(hinv, what):
    assert bool((hinv > 0).all()) and bool(torch.isfinite(hinv).all()), f"{what}: hinv {hinv.tolist()}"
    m, _ = torch.frexp(hinv)
    assert bool((m == 0.5).all()), f"{what}: hinv is no power of two: {hinv.tolist()}"


def assert_u_of_launch(res, n_owned, what):
    """The host-count checks of a fp16x2w launch with n_owned proposals: tail rows zero, owned rows sane."""
    mblocks = (n_owned + 7) // 8
    hi, lo, hinv = decode_U(res["ws"], res["n"], mblocks)
    assert guard_intact(res), f"{what}: the guard band behind the workspace was written"
    tail = slice(16 * n_owned, None)
    assert is_zero_bits(hi[tail]) and is_zero_bits(lo[tail]), f"{what}: rows of proposals {n_owned}..{8 * mblocks - 1} are not zero bits"
    assert is_zero_bits(hinv[n_owned:]), f"{what}: hinv behind the last proposal is not 0.0"
    assert_planes_sane(hi[:16 * n_owned], lo[:16 * n_owned], 2.0 ** 13, what)
    assert_pow2(hinv[:n_owned], what)
    return hi, lo, hinv


# ---- the launches and checks the two test files share ----------------------------------------------------------------------
# platform -> pair size, proposal counts of the host-count launches, the big launch, the single-proposal launches it is
# compared with, the prefix launch
CONFIG = {
    "emu": dict(H=16, W=24, ns=(1, 9), big=9, singles=(0, 8), prefix=None),
    "gpu": dict(H=64, W=96, ns=(1, 7, 9, 41), big=41, singles=(0, 7, 8, 40), prefix=9),
}
DEV_COUNT_SIZES = ((16, 24), (24, 16), (8, 8), (16, 16))      # image sizes of the items of a device-count call


def proposals(H, W, n, seed=5):
    """int64 [n,4]: two opposite image corners first, the rest seeded."""
    g = torch.Generator().manual_seed(seed)
    p = torch.stack([torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g),
                     torch.randint(0, W + 1, (n,), generator=g), torch.randint(0, H + 1, (n,), generator=g)], 1)
    p[0] = torch.tensor([0, 0, W, H])
    if n > 1:
        p[1] = torch.tensor([W, 0, 0, H])
    return p


class FineLaunches:
    """The launches of one pair, made on demand and kept: get(mode, lo, hi, two) = props[lo:hi] through mid (+ fine)."""

    def __init__(self, platform, lib, dev, handles):
        from patch2pix_amd.utils import synthetic
        c = CONFIG[platform]
        self.platform, self.lib, self.dev, self.handles, self.cfg = platform, lib, dev, handles, c
        self.pyr1, self.pyr2 = synthetic.make_pyramid(71, c["H"], c["W"])[:4], synthetic.make_pyramid(72, c["H"], c["W"])[:4]
        self.props = proposals(c["H"], c["W"], c["big"])
        self._done = {}

    def get(self, mode, lo, hi, two):
        key = (mode, lo, hi, two)
        if key not in self._done:
            mid, fine = self.handles[mode]
            self._done[key] = run_fine(self.lib, mid, fine if two else None, self.pyr1, self.pyr2, self.props[lo:hi], self.dev)
        return self._done[key]


def check_workspace_formulas(lib, ncn, modes):
    """The restated carve-up gives the library's totals (fine: both two-plane modes; coarse: a tuned consensus handle)."""
    for n in (1, 7, 8, 9, 41, 255, 256, 3327, 3328, 3329, 3403, 6400):
        for mode, code in modes.items():
            if mode != "f32":
                assert regress_ws_bytes(n, mode) == lib.p2p_regress_workspace_bytes_mode(n, code), (n, mode)
    assert wino_chunks(3403) == [(0, 1792), (1792, 3403)] and wino_chunks(6400) == [(0, 3328), (3328, 6400)]
    for (C, ha, wa, hb, wb, k) in COARSE_CASES + ((256, 30, 40, 30, 40, 2), (32, 16, 16, 12, 20, 4)):
        assert coarse_ws_offsets(C, ha, wa, hb, wb, k)["total"] == lib.p2p_coarse_workspace_bytes_for(ncn, C, ha, wa, hb, wb, k)


def check_host_counts(L, n, two):
    """A host-count fp16x2w launch of n proposals (after a two-level call U holds level 2): section 2 of the list."""
    res = L.get("fp16x2w", 0, n, two)
    what = f"n = {n}, {'two levels' if two else 'one level'}"
    assert_u_of_launch(res, n, what)
    for lvl in range(2 if two else 1):
        v = decode_V(res["ws"], n, lvl)
        assert bool(torch.isfinite(v).all()) and bool((v >= 0).all()), f"{what}: V of level {lvl + 1}"
    if not two:
        assert is_poison(decode_V(res["ws"], n, 1)), f"{what}: V of the level that did not run was written"
    assert not bool((res["matches1"] == MARK).any())


def check_independence(L, i, lo=None, hi=None):
    """Proposal i of the big launch against the launch props[lo:hi] (default: i alone): U rows, hinv and V bit for bit in
    the one-level call, V of both levels in the two-level chain."""
    big = L.cfg["big"]
    lo, hi = (i, i + 1) if lo is None else (lo, hi)
    a1, b1 = L.get("fp16x2w", 0, big, False), L.get("fp16x2w", lo, hi, False)
    ua, ub = decode_U(a1["ws"], big, (big + 7) // 8, [i]), decode_U(b1["ws"], hi - lo, (hi - lo + 7) // 8, [i - lo])
    for x, y, name in zip(ua, ub, ("U hi", "U lo", "hinv")):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x, y.view(torch.int16) if y.dtype == torch.float16 else y), \
            f"proposal {i}: {name} differs between the launch of {big} and the launch [{lo}, {hi})"
    assert torch.equal(decode_V(a1["ws"], big, 0)[i], decode_V(b1["ws"], hi - lo, 0)[i - lo]), f"proposal {i}: V (one level)"
    a2, b2 = L.get("fp16x2w", 0, big, True), L.get("fp16x2w", lo, hi, True)
    for lvl in (0, 1):
        assert torch.equal(decode_V(a2["ws"], big, lvl)[i], decode_V(b2["ws"], hi - lo, lvl)[i - lo]), f"proposal {i}: V of level {lvl + 1}"
    for k in ("matches1", "probs1", "matches2", "probs2"):
        assert torch.equal(a2[k][i], b2[k][i - lo]), f"proposal {i}: {k}"


def check_device_counts(lib, dev, mid, fine, stride, counts):
    """p2p_regress_batch_dev, two levels, mode fp16x2w.  U and hinv are indexed by the COMPACT proposal number (item
    order, the first counts[i] slots of every item); the rows behind the last compact proposal of its row block are
    zero; owned rows equal the per-item call bit for bit; V rows and outputs of unowned slots keep the poison / the mark.
    Row blocks past the last compact proposal stay POISONED, all of them: wino_zero_tail_kernel and wino_gemm_kernel
    both leave a block none of whose proposals exists (asserted as "all poison or all zero" per block, and then as poison)."""
    from patch2pix_amd.utils import synthetic
    items = len(counts)
    sizes = [DEV_COUNT_SIZES[i % len(DEV_COUNT_SIZES)] for i in range(items)]
    pyr1 = [synthetic.make_pyramid(200 + i, h, w)[:4] for i, (h, w) in enumerate(sizes)]
    pyr2 = [synthetic.make_pyramid(300 + i, h, w)[:4] for i, (h, w) in enumerate(sizes)]
    props = torch.zeros(items, stride, 4, dtype=torch.int64)
    for i, (h, w) in enumerate(sizes):
        props[i] = proposals(h, w, stride, seed=40 + i)
    n = items * stride
    res = run_fine(lib, mid, fine, pyr1, pyr2, props.reshape(n, 4), dev, counts=list(counts), stride=stride)
    assert guard_intact(res)
    mblocks = (n + 7) // 8
    hi, lo, hinv = decode_U(res["ws"], n, mblocks)
    own = [max(0, min(c, stride)) for c in counts]
    total = sum(own)
    assert total > 0
    c0 = 0
    for i, c in enumerate(own):
        used, rest = slice(i * stride, i * stride + c), slice(i * stride + c, (i + 1) * stride)
        for lvl in (0, 1):
            assert is_poison(decode_V(res["ws"], n, lvl)[rest]), f"item {i}: V rows of empty slots were written (level {lvl + 1})"
        for k in ("matches1", "probs1", "matches2", "probs2"):
            assert bool((res[k][rest] == MARK).all()), f"item {i}: {k} of empty slots"
        if not c:
            continue
        one = run_fine(lib, mid, fine, pyr1[i], pyr2[i], props[i, :c], dev)
        shi, slo, shinv = decode_U(one["ws"], c, (c + 7) // 8)
        rows = slice(16 * c0, 16 * (c0 + c))
        assert torch.equal(_bits(hi[rows]), _bits(shi[:16 * c])) and torch.equal(_bits(lo[rows]), _bits(slo[:16 * c])), \
            f"item {i}: U rows of compact proposals {c0}..{c0 + c - 1} differ from the item's own call"
        assert torch.equal(hinv[c0:c0 + c], shinv[:c]), f"item {i}: hinv"
        for lvl in (0, 1):
            assert torch.equal(decode_V(res["ws"], n, lvl)[used], decode_V(one["ws"], c, lvl)), f"item {i}: V of level {lvl + 1}"
        for k in ("matches1", "probs1", "matches2", "probs2"):
            assert torch.equal(res[k][used], one[k]), f"item {i}: {k}"
        c0 += c
    filled = (total + 7) // 8
    assert is_zero_bits(hi[16 * total:128 * filled]) and is_zero_bits(lo[16 * total:128 * filled]), "rows behind the last compact proposal of its block"
    assert is_zero_bits(hinv[total:8 * filled])
    assert_planes_sane(hi[:16 * total], lo[:16 * total], 2.0 ** 13, "device counts")
    assert_pow2(hinv[:total], "device counts")
    for mb in range(filled, mblocks):
        blk = (hi[128 * mb:128 * (mb + 1)], lo[128 * mb:128 * (mb + 1)], hinv[8 * mb:8 * (mb + 1)])
        assert all(is_poison(t) for t in blk) or all(is_zero_bits(t) for t in blk), f"row block {mb}: partly written"
        assert all(is_poison(t) for t in blk), f"row block {mb} (past the last compact proposal) was written"


def measure_fine(L, mode, sd):
    """Section 3 on the big launch of L: {(metric, level): (e kernel, e fp32 restatement)}, each the worst proposal, both
    against fp64.  Level 2 (index 1) of every reference is fed the kernel's own mid matches.  No proposal and no channel
    is left out."""
    big = L.cfg["big"]
    _, mid_p, fine_p = orc.split_params(sd)
    two = L.get(mode, 0, big, True)
    feeds = [(L.props, mid_p), (two["matches1"].cpu(), fine_p)]
    out = {}
    for lvl, (m, prm) in enumerate(feeds):
        _, u64, v64 = fine_stages(L.pyr1, L.pyr2, m, prm, torch.float64)
        _, u32, v32 = fine_stages(L.pyr1, L.pyr2, m, prm, torch.float32)
        out[("V", lvl)] = (float(e_V(decode_V(two["ws"], big, lvl).cpu(), v64).max()), float(e_V(v32, v64).max()))
        if mode == "fp16x2w":
            res = two if lvl == 1 else L.get(mode, 0, big, False)
            hi, lo, hinv = (t.cpu() for t in decode_U(res["ws"], big, (big + 7) // 8))
            one = torch.ones(big, dtype=torch.float64)
            zero = torch.zeros_like(u32, dtype=torch.float32)
            out[("U", lvl)] = (float(e_U(hi[:16 * big], lo[:16 * big], hinv, u64).max()), float(e_U(u32, zero, one, u64).max()))
    return out


def assert_fine_values(L, mode, sd, label=None):
    fig = measure_fine(L, mode, sd)
    for (metric, lvl), (ek, e32) in sorted(fig.items()):
        print(f"\nstage[{label or L.platform}] {mode:>8s} e_{metric} level {lvl + 1}: kernel {ek:.3e}  fp32 restatement {e32:.3e}  r = {ek / e32:.3f}")
    for (metric, lvl), (ek, e32) in sorted(fig.items()):
        b = bar(L.platform, mode, metric, lvl)
        assert ek <= b * e32, f"{mode} e_{metric} level {lvl + 1}: {ek:.3e} > {b} x {e32:.3e}"
    return fig


# coarse cases: (C, hA, wA, hB, wB, ksize): h * w no multiple of 128 on either image, different sizes; ksize 4: h * w = 16 x odd
COARSE_CASES = ((96, 6, 8, 9, 7, 1), (96, 6, 8, 10, 6, 2), (64, 4, 12, 8, 8, 4))
COARSE_PAIRS = 3


def coarse_features(case, seed=3, scale=1.0):
    C, ha, wa, hb, wb, _ = case
    g = torch.Generator().manual_seed(seed)
    return (torch.relu(torch.randn(COARSE_PAIRS, C, ha, wa, generator=g) + 0.3) * scale,
            torch.relu(torch.randn(COARSE_PAIRS, C, hb, wb, generator=g) + 0.3) * scale)


def coarse_planes(lib, dev, ncn, case, fa, fb):
    """run_coarse + decode: -> (res, {(pair, image): (hi, lo)}); asserts the guard band and the untouched bytes between the
    last block of a plane and the next part of the carve-up."""
    C, ha, wa, hb, wb, k = case
    res = run_coarse(lib, ncn, fa, fb, k, dev)
    off = coarse_ws_offsets(C, ha, wa, hb, wb, k)
    assert off["total"] == res["per_pair"]
    assert guard_intact(res), "the guard band behind the coarse workspace was written"
    planes = {}
    for z in range(fa.shape[0]):
        for img, (h, w, name, nxt) in enumerate(((ha, wa, "fnA", "fnB"), (hb, wb, "fnB", "P"))):
            planes[(z, img)] = decode_planes(res["ws"][z], C, h, w, k, img, off[name])
            gap = res["ws"][z][off[name] + _up(h * w, 128) * C * 4:off[nxt]]
            assert is_poison(gap), f"pair {z}: bytes between the last block of {name} and {nxt} were written"
    return res, planes


def check_coarse_case(lib, dev, ncn, case, platform):
    """Pad rows zero in both planes and all chunks, live rows sane, canonical and bounded, e_F at its bar."""
    C, ha, wa, hb, wb, k = case
    fa, fb = coarse_features(case)
    _, planes = coarse_planes(lib, dev, ncn, case, fa, fb)
    worst = [0.0, 0.0]
    for (z, img), (hi, lo) in planes.items():
        feat, hw = ((fa, ha * wa), (fb, hb * wb))[img]
        what = f"case {case} pair {z} image {img}"
        assert hi.shape[0] > hw and is_zero_bits(hi[hw:]) and is_zero_bits(lo[hw:]), f"{what}: pad rows are not zero bits"
        assert_planes_sane(hi[:hw], lo[:hw], 4096.0 * (1 + 2.0 ** -10), what, strict=False)
        f64 = coarse_planes_ref(feat[z], torch.float64)
        got = (hi[:hw].double() + lo[:hw].double()).cpu() / 4096.0
        assert bool((got.abs().amax(1) > 0).all()), f"{what}: a live row is zero"
        worst[0] = max(worst[0], float((got - f64).abs().max()))
        worst[1] = max(worst[1], float((coarse_planes_ref(feat[z], torch.float32).double() - f64).abs().max()))
    print(f"\nstage[{platform}] coarse {case}: e_F kernel {worst[0]:.3e}  fp32 restatement {worst[1]:.3e}  r = {worst[0] / worst[1]:.3f}")
    b = bar(platform, "coarse", "F", case[5])
    assert worst[0] <= b * worst[1], f"e_F {worst[0]:.3e} > {b} x {worst[1]:.3e}"


def check_coarse_scale_free(lib, dev, ncn, case):
    """Features x 2^7 -> the same plane bits: every fp32 operation of the normalisation scales exactly, and at these
    magnitudes (sum of squares >= 64, asserted) ss + 1e-6 == ss in fp32."""
    fa, fb = coarse_features(case, scale=16.0)
    for f in (fa, fb):
        ss = (f * f).sum(1)
        assert float(ss.min()) >= 64.0 and bool(((ss + 1e-6) == ss).all())
    _, p1 = coarse_planes(lib, dev, ncn, case, fa, fb)
    _, p2 = coarse_planes(lib, dev, ncn, case, fa * 128.0, fb * 128.0)
    for key in p1:
        for a, b in zip(p1[key], p2[key]):
            assert torch.equal(_bits(a), _bits(b)), f"pair / image {key}: scaling the features by 2^7 changes the planes"


def check_coarse_zero_column(lib, dev, ncn, case):
    """Positions whose features are all zero give exactly-zero rows in both planes (0 x 1/sqrt(1e-6)), not NaN."""
    C, ha, wa, hb, wb, k = case
    fa, fb = coarse_features(case)
    dead_a, dead_b = [0, ha * wa - 1, 5], [1, hb * wb - 1]
    fa.reshape(COARSE_PAIRS, C, -1)[1][:, dead_a] = 0.0
    fb.reshape(COARSE_PAIRS, C, -1)[1][:, dead_b] = 0.0
    res, planes = coarse_planes(lib, dev, ncn, case, fa, fb)
    for img, dead in ((0, dead_a), (1, dead_b)):
        hi, lo = planes[(1, img)]
        assert is_zero_bits(hi[dead]) and is_zero_bits(lo[dead]), f"image {img}: rows of all-zero positions"
        hw = (ha * wa, hb * wb)[img]
        keep = torch.ones(hw, dtype=torch.bool)
        keep[dead] = False
        assert bool((hi[:hw][keep.to(hi.device)].float().abs().amax(1) > 0).all())
    assert bool(torch.isfinite(res["corr"]).all())
