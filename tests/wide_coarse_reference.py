"""TEST INFRASTRUCTURE: the coarse stage at up to 1024 channels (the layer-3 width of a Bottleneck backbone) -- the case table,
the seeded inputs and the assertions shared by tests/test_wide_coarse_emulated.py (the kernels' code on the CPU, tests/hipemu),
tests/test_gpu_wide_coarse.py (MI355X) and tests/make_golden_wide_coarse.py.

Everything numeric is tests/coarse_mode_reference.py's (the fp64 `Yardstick`, its element-wise bounds, `check_stages`,
`check_rows`): every bound there already takes the reduction length K from the channel count of its inputs.  The cases of this
file are registered in that module's case table under their own names, with their yardsticks built here from inputs that carry
their OWN seeds (the seeds of that module follow a case's position in its table).

BOUNDS added here.
  operand planes   (hi + lo) / 2^12 against the fp64 normalisation n: the fp32 normalisation is within ENORM |n|,
                   ENORM = (0.5 (C + 2) + 4) 2^-24 (coarse_mode_reference.py, "normalise"), and the two-plane split of the fp32
                   value x = n 2^12 is within max(2^-24 |x|, 2^-24) (the figure the sources state for the split, with the fp16
                   subnormal spacing as its absolute floor): |decoded - n| <= ENORM |n| + operand_error(|n| (1 + ENORM), 2^12, 2^-24).
                   Mode 'fp16' (one plane): the same with 2^-11.
  pooled volume    oracle/error_model.py's ErrorModel takes K = C from its inputs as well: its `check` (the volume within
                   CHECK_LIMIT x the propagated fp32 bound) runs on the final volume of every case in the default mode.
  undecided rows   the share of coarse rows the kernel's bound cannot decide must not exceed the share an fp32 evaluation
                   leaves undecided under ErrorModel on the same inputs (`assert_undecided_share`): a condition on the seeds,
                   computed on the CPU, not a tolerance."""
import torch

import coarse_mode_reference as cm
from oracle import error_model as em

# name -> (C, (hA, wA), (hB, wB), ksize, pairs, gpu_only), seed
WIDE = {
    "w32_4x6_6x4_k2": ((32, (4, 6), (6, 4), 2, 1, False), 9101),
    "w256_4x6_6x4_k2": ((256, (4, 6), (6, 4), 2, 1, False), 9102),
    "w288_4x6_6x4_k2": ((288, (4, 6), (6, 4), 2, 1, False), 9103),          # the first width of the dynamic tile; 9 K chunks (odd)
    "w1024_4x6_6x4_k2": ((1024, (4, 6), (6, 4), 2, 1, False), 9104),
    "w1024_4x6_6x4_k1": ((1024, (4, 6), (6, 4), 1, 1, False), 9105),
    "w1024_4x6_6x4_k2_batch3": ((1024, (4, 6), (6, 4), 2, 3, False), 9106),  # magnitudes 1, 2^10, 2^-10; pair 1 has dead cells
}
GOLDEN_CASES = ["w32_4x6_6x4_k2", "w256_4x6_6x4_k2"]              # recorded from the library that stopped at 256 channels
NEW_CASES = ["w288_4x6_6x4_k2", "w1024_4x6_6x4_k2", "w1024_4x6_6x4_k1"]
BATCH_CASE = "w1024_4x6_6x4_k2_batch3"
GOLDEN_FILE = "wide_coarse_parent"

for _name, (_case, _seed) in WIDE.items():
    cm.CASES.setdefault(_name, _case)

_inputs = {}


def case_inputs(name):
    """Seeded planted features (fa [B,C,hA,wA], fb [B,C,hB,wB]) of a case: a cell of B is a cell of A with its k x k positions
    shuffled, plus noise (coarse_mode_reference.case_inputs' construction under this file's seeds)."""
    if name in _inputs:
        return _inputs[name]
    (c, (ha, wa), (hb, wb), k, pairs, _), seed = WIDE[name]
    gen = torch.Generator().manual_seed(seed)
    fa = torch.randn(pairs, c, ha * wa, generator=gen)
    fb = torch.empty(pairs, c, hb * wb)
    nac, nbc, wac, wbc = (ha // k) * (wa // k), (hb // k) * (wb // k), wa // k, wb // k
    for z in range(pairs):
        cell = torch.cat([torch.randperm(nac, generator=gen) for _ in range((nbc + nac - 1) // nac)])[:nbc]
        src = torch.empty(hb * wb, dtype=torch.long)
        for cb in range(nbc):
            ca, sub = int(cell[cb]), torch.randperm(k * k, generator=gen)
            for q in range(k * k):
                qa = int(sub[q])
                src[((cb // wbc) * k + q // k) * wb + (cb % wbc) * k + q % k] = ((ca // wac) * k + qa // k) * wa + (ca % wac) * k + qa % k
        fb[z] = fa[z][:, src] + 0.3 * torch.randn(c, hb * wb, generator=gen)
    if pairs == 3:
        mag = torch.tensor([1.0, 1024.0, 1.0 / 1024.0]).view(3, 1, 1)
        fa, fb = fa * mag, fb * mag
        fa.view(pairs, c, ha, wa)[1, :, 2:4, 2:4] = 0.0        # a block of exact zeros: one dead pooling cell
    _inputs[name] = (fa.view(pairs, c, ha, wa).contiguous(), fb.view(pairs, c, hb, wb).contiguous())
    return _inputs[name]


def yardsticks(name, sd, mode):
    """The case's fp64 yardsticks, placed where coarse_mode_reference's assertions look them up."""
    key = (name, mode)
    if key not in cm._yard_cache:
        fa, fb = case_inputs(name)
        cm._yard_cache[key] = [cm.Yardstick(fa[z], fb[z], WIDE[name][0][3], sd, mode) for z in range(fa.shape[0])]
    return cm._yard_cache[key]


_models = {}


def error_models(name, sd):
    """oracle/error_model.py's fp64 evaluation + propagated fp32 bound per pair (K = C from the inputs)."""
    if name not in _models:
        fa, fb = case_inputs(name)
        _models[name] = [em.ErrorModel(fa[z], fb[z], sd, ksize=WIDE[name][0][3]) for z in range(fa.shape[0])]
    return _models[name]


def assert_undecided_share(name, sd, mode="fp16x2"):
    """-> (share of rows the kernel's bound leaves undecided, share ErrorModel leaves undecided for an fp32 evaluation)."""
    mine = torch.cat([~y.decidable()[1] for y in yardsticks(name, sd, mode)]).double().mean().item()
    ref = torch.cat([~m.decidable()[1] for m in error_models(name, sd)]).double().mean().item()
    assert mine <= ref, f"{name}: {mine:.3f} of the rows are undecided under the kernel's bound, {ref:.3f} under the fp32 error model"
    return mine, ref


def run(lib, sd, name, mode=None, pair=None, ws_pairs=None, dev="cpu", stream=None):
    """One coarse stage of a case on a fresh handle of `lib` (emulated or real) -> coarse_mode_reference.run_coarse's dict
    plus rows / scores of p2p_coarse_matches_batch."""
    fa, fb = case_inputs(name)
    if pair is not None:
        fa, fb = fa[pair:pair + 1], fb[pair:pair + 1]
    ncn = cm.ncn_create(lib, sd)
    try:
        if mode is not None:
            cm.set_mode(lib, ncn, mode)
        k = WIDE[name][0][3]
        out = cm.run_coarse(lib, ncn, fa.to(dev), fb.to(dev), k, ws_pairs=ws_pairs, stream=stream)
        out["rows"], out["scores"] = cm.run_matches(lib, out["corr"], out["delta"], k, stream=stream)
    finally:
        lib.p2p_ncn_destroy(ncn)
    return out


def planes_of(lib, sd, name, mode, dev="cpu"):
    """{(pair, image): (hi, lo) fp16 [rows, C]} of a case through stage_reference's poisoned-workspace driver and decoder.
    Mode 'fp16' fills the first half of the two-plane sized buffers with single-plane blocks: decoded here as [.., 1, ..]."""
    import stage_reference as sr
    fa, fb = case_inputs(name)
    c, (ha, wa), (hb, wb), k, _, _ = WIDE[name][0]
    ncn = cm.ncn_create(lib, sd)
    try:
        if mode != "fp16x2":
            cm.set_mode(lib, ncn, mode)
        res = sr.run_coarse(lib, ncn, fa, fb, k, dev)
    finally:
        lib.p2p_ncn_destroy(ncn)
    assert sr.guard_intact(res), "the guard band behind the coarse workspace was written"
    off = sr.coarse_ws_offsets(c, ha, wa, hb, wb, k)
    assert off["total"] == res["per_pair"]
    planes = {}
    for z in range(fa.shape[0]):
        for img, (h, w, key) in enumerate(((ha, wa, "fnA"), (hb, wb, "fnB"))):
            if mode == "fp16x2":
                planes[(z, img)] = sr.decode_planes(res["ws"][z], c, h, w, k, img, off[key])
            else:
                nblk = (h * w + 127) // 128
                raw = res["ws"][z][off[key]:off[key] + nblk * 128 * c * 2].view(torch.int16).view(nblk, c // 32, 1, 128, 4, 8)
                v = sr._unswizzle(raw).permute(0, 3, 2, 1, 4, 5).reshape(nblk * 128, c)
                live = sr.plane_row(torch.arange(h * w, device=v.device), h, w, k, img)
                hi = v[live].contiguous().view(torch.float16)
                planes[(z, img)] = (hi, torch.zeros_like(hi))
    return res, planes


def check_planes(planes, name, mode, what=""):
    """Every live row within the derived operand bound of the fp64 normalisation (module docstring); pad rows zero bits (two
    planes).  -> largest error / bound."""
    import stage_reference as sr
    fa, fb = case_inputs(name)
    c = fa.shape[1]
    enorm = (0.5 * (c + 2) + 4) * cm.U32
    worst = 0.0
    for (z, img), (hi, lo) in planes.items():
        feat = (fa, fb)[img][z]
        hw = feat.shape[1] * feat.shape[2]
        n64 = sr.coarse_planes_ref(feat, torch.float64)
        got = (hi[:hw].double() + lo[:hw].double()).cpu() / 4096.0
        bound = enorm * n64.abs() + cm.operand_error(n64.abs() * (1 + enorm), 4096.0, cm.EPS[mode])
        err = (got - n64).abs()
        assert bool(torch.isfinite(got).all())
        ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f"{what}{name} pair {z} image {img} mode {mode}: plane error {ratio:.3f} of its bound"
        if mode == "fp16x2":
            assert sr.is_zero_bits(hi[hw:]) and sr.is_zero_bits(lo[hw:]), f"{what}{name} pair {z} image {img}: pad rows are not zero bits"
    print(f"{what}{name} mode {mode}: operand planes, max err / bound {worst:.4f}")
    return worst


def check_error_model(out, name, sd, what=""):
    """The final volume within CHECK_LIMIT x oracle/error_model.py's fp32 bound propagated for K = C; every row that model can
    decide names the fp64 winner (cells and, for ksize > 1, the relocalisation)."""
    worst = 0.0
    for z, model in enumerate(error_models(name, sd)):
        worst = max(worst, model.check(out["corr"][z].detach().cpu(), f"{what}{name}[{z}]"))
        em.assert_decidable_rows(out["rows"][z].detach().cpu(), model, upsample=8)
    print(f"{what}{name}: |error| / fp32 error model {worst:.3f} (limit {em.CHECK_LIMIT})")
    return worst
