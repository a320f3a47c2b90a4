"""The coarse stage at up to 1024 channels on the MI355X through the real library: the assertions of
tests/test_wide_coarse_emulated.py (bounds, decidable rows, batch independence) plus a larger volume whose correlation GEMM has
several tiles and all 32 K chunks.  Cases and helpers: tests/wide_coarse_reference.py."""
import ctypes

import pytest
import torch

import coarse_mode_reference as cm
import golden_util as gu
import wide_coarse_reference as wc
from oracle import error_model as em
from oracle import p2p_oracle as orc

pytestmark = pytest.mark.gpu
MODES = ("fp16x2", "fp16")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from patch2pix_amd import _lib
    return _lib.lib


def _sd():
    return gu.state_dict(0)


_CACHE = {}


def _run(lib, dev, name, mode="fp16x2", pair=None, ws_pairs=None):
    key = (name, mode, pair, ws_pairs)
    if key not in _CACHE:
        with torch.cuda.device(dev):
            out = wc.run(lib, _sd(), name, mode, pair, ws_pairs, dev=dev, stream=torch.cuda.current_stream(dev).cuda_stream)
        _CACHE[key] = {k: (v.cpu() if v is not None else None) for k, v in out.items()}
    return _CACHE[key]


@pytest.mark.parametrize("name", wc.GOLDEN_CASES + wc.NEW_CASES)
def test_stage_bounds_and_rows(name, lib, dev):
    sd = _sd()
    wc.assert_undecided_share(name, sd)
    for mode in MODES:
        wc.yardsticks(name, sd, mode)
        out = _run(lib, dev, name, mode)
        ratios = cm.check_stages(out, name, sd, mode, "MI355X ")
        bad, dec, tot = cm.check_rows(out["rows"], name, sd, mode)
        print(f"MI355X {name} mode {mode}: measured / bound {ratios}; {dec} / {tot} rows decidable, {bad} differ from fp64")
    wc.check_error_model(_run(lib, dev, name), name, sd, "MI355X ")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", wc.NEW_CASES)
def test_planes(name, mode, lib, dev):
    with torch.cuda.device(dev):
        _, planes = wc.planes_of(lib, _sd(), name, mode, dev=dev)
    wc.check_planes({k: (hi.cpu(), lo.cpu()) for k, (hi, lo) in planes.items()}, name, mode, "MI355X ")


@pytest.mark.parametrize("mode", MODES)
def test_batch_and_workspace_independence_at_1024_channels(mode, lib, dev):
    name = wc.BATCH_CASE
    batch, small = _run(lib, dev, name, mode), _run(lib, dev, name, mode, None, 1)
    for key in ("corr", "delta", "rows", "scores"):
        assert torch.equal(small[key], batch[key]), key
    for z in range(3):
        one = _run(lib, dev, name, mode, z)
        for key in ("corr", "delta", "x", "y", "rows", "scores"):
            assert torch.equal(one[key][0], batch[key][z]), f"pair {z}: {key}"
    wc.yardsticks(name, _sd(), mode)
    cm.check_stages(batch, name, _sd(), mode, "MI355X ")


@pytest.mark.parametrize("ksize", [1, 2])
def test_several_tiles_at_1024_channels(ksize, lib, dev):
    """16 x 20 against 20 x 16 positions (320 rows: three tiles a side, the last one partial) at 1024 channels, two pairs,
    against the fp32 error model of the fp64 evaluation and the oracle's rows."""
    from patch2pix_amd import ops
    g = torch.Generator().manual_seed(77 + ksize)
    fa = torch.relu(torch.randn(2, 1024, 16, 20, generator=g) - 0.8)
    perm = torch.randperm(320, generator=g)
    fb = torch.relu(fa.reshape(2, 1024, 320)[:, :, perm].reshape(2, 1024, 20, 16) + 0.2 * torch.randn(2, 1024, 20, 16, generator=g))
    sd = _sd()
    ncn = ops.NcnWeights.from_state_dict({k[len("ncn."):]: v for k, v in sd.items() if k.startswith("ncn.")}, dev)
    corr, delta = ops.coarse_forward_batch(fa.to(dev), fb.to(dev), ksize, ncn)
    rows, scores = ops.coarse_matches_batch(corr, delta, ksize, 8, True)
    one, _ = ops.coarse_forward_batch(fa[1:].to(dev), fb[1:].to(dev), ksize, ncn)
    assert torch.equal(one[0], corr[1])
    for z in range(2):
        model = em.ErrorModel(fa[z], fb[z], sd, ksize=ksize, keep_full=False)
        ratio = model.check(corr[z].cpu(), f"pair {z}")
        ndec, nrows = em.assert_decidable_rows(rows[z].cpu(), model, 8)
        print(f"1024 channels ksize {ksize} pair {z}: |error| / fp32 model {ratio:.3f}, {ndec} of {nrows} rows decidable")
        assert ndec > 0


def test_channel_limit(lib, dev):
    fa = torch.zeros(1, 1056, 4, 6, device=dev)
    out = torch.zeros(1, 2, 3, 2, 3, device=dev)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ncn = cm.ncn_create(lib, _sd())
        try:
            for c in (1056, 1030):
                st = lib.p2p_coarse_forward_batch(ctypes.c_void_p(fa.data_ptr()), ctypes.c_void_p(fa.data_ptr()), 1, c, 4, 6, 4, 6, 2, ncn,
                                                  ctypes.c_void_p(out.data_ptr()), None, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
                assert st == -3 and b"1024" in lib.p2p_last_error()
        finally:
            lib.p2p_ncn_destroy(ncn)
