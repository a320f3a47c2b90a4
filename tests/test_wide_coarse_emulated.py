"""The coarse stage at up to 1024 channels on the CPU build of the kernels (tests/hipemu); cases, bounds and helpers in
tests/wide_coarse_reference.py.  At 32 and 256 channels the operand buffers and every output must be the bits the library gave
before the preparation kernel learnt more than 256 channels (tests/golden/wide_coarse_parent.npz); at 288 and 1024 channels the
planes, the stage volumes and the decidable rows are held to the derived bounds; a pair at 1024 channels is bit-equal alone, in
a batch of 3 and with a one-pair workspace.  tests/test_gpu_wide_coarse.py asserts the same on the MI355X."""
import ctypes
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import golden_util as gu  # noqa: E402
import coarse_mode_reference as cm  # noqa: E402
import stage_reference as sr  # noqa: E402
import wide_coarse_reference as wc  # noqa: E402

MODES = ("fp16x2", "fp16")


@functools.lru_cache(maxsize=None)
def _emu():
    return cm.bind(emu_lib.load())


def _sd():
    return gu.state_dict(0)


@functools.lru_cache(maxsize=None)
def _run(name, mode="fp16x2", pair=None, ws_pairs=None):
    return wc.run(_emu(), _sd(), name, mode, pair, ws_pairs)


@functools.lru_cache(maxsize=None)
def _planes(name, mode):
    return wc.planes_of(_emu(), _sd(), name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", wc.GOLDEN_CASES)
def test_up_to_256_channels_keep_their_bits(name, mode):
    """Feature planes (raw bytes of both buffers) and every stage output equal the recorded ones bit for bit."""
    g = gu.load(wc.GOLDEN_FILE)
    pre = f"{name}/{mode}/"
    fa, fb = wc.case_inputs(name)
    assert abs(gu.checksum([fa, fb]) - float(g[pre + "input_checksum"])) <= 1e-9 * float(g[pre + "input_checksum"]), "the seeded inputs drifted"
    c, (ha, wa), (hb, wb), k, _, _ = wc.WIDE[name][0]
    res, _ = _planes(name, mode)
    off = sr.coarse_ws_offsets(c, ha, wa, hb, wb, k)
    for key, n in (("fnA", ha * wa), ("fnB", hb * wb)):
        want = torch.from_numpy(g[pre + key])
        got = res["ws"][0][off[key]:off[key] + want.numel()]
        assert torch.equal(got, want), f"{name} mode {mode}: the bytes of {key} changed"
    out = _run(name, mode)
    for key in ("x", "y", "corr", "delta", "rows", "scores"):
        want = torch.from_numpy(g[pre + key])
        assert out[key].dtype == want.dtype and torch.equal(out[key], want), f"{name} mode {mode}: {key} changed"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", wc.NEW_CASES + [wc.BATCH_CASE])
def test_planes_decode_to_the_fp64_normalisation(name, mode):
    _, planes = _planes(name, mode)
    wc.check_planes(planes, name, mode, "emulated ")
    if mode == "fp16x2":
        for (z, img), (hi, lo) in planes.items():
            hw = wc.case_inputs(name)[img].shape[2] * wc.case_inputs(name)[img].shape[3]
            sr.assert_planes_sane(hi[:hw], lo[:hw], 4096.0 * (1 + 2.0 ** -10), f"{name} pair {z} image {img}", strict=False)


@pytest.mark.parametrize("name", wc.NEW_CASES)
def test_stage_bounds_and_rows_in_both_modes(name):
    """Every stage volume within its element-wise bound for K = C in both modes; every decidable row names the fp64 winner; the
    share of undecided rows is no larger than an fp32 evaluation's; the default mode also inside oracle/error_model.py."""
    sd = _sd()
    mine, ref = wc.assert_undecided_share(name, sd)
    print(f"emulated {name}: undecided rows {mine:.3f} (kernel bound) / {ref:.3f} (fp32 error model)")
    for mode in MODES:
        wc.yardsticks(name, sd, mode)
        out = _run(name, mode)
        ratios = cm.check_stages(out, name, sd, mode, "emulated ")
        bad, dec, tot = cm.check_rows(out["rows"], name, sd, mode)
        print(f"emulated {name} mode {mode}: measured / bound {ratios}; {dec} / {tot} rows decidable, {bad} differ from fp64")
    wc.check_error_model(_run(name), name, sd, "emulated ")
    assert not torch.equal(_run(name)["corr"], _run(name, "fp16")["corr"]), "mode 'fp16' gave the default mode's bits"


@pytest.mark.parametrize("mode", MODES)
def test_batch_and_workspace_independence_at_1024_channels(mode):
    """A pair alone == the pair in a batch of 3 == the batch through a one-pair workspace, bit for bit (planes included)."""
    name = wc.BATCH_CASE
    batch = _run(name, mode)
    small = _run(name, mode, None, 1)
    assert torch.equal(small["corr"], batch["corr"]) and torch.equal(small["delta"], batch["delta"])
    assert torch.equal(small["rows"], batch["rows"]) and torch.equal(small["scores"], batch["scores"])
    _, planes = _planes(name, mode)
    c, (ha, wa), (hb, wb), k, _, _ = wc.WIDE[name][0]
    fa, fb = wc.case_inputs(name)
    emu, ncn = _emu(), cm.ncn_create(_emu(), _sd())
    try:
        cm.set_mode(emu, ncn, mode)
        for z in range(3):
            one = _run(name, mode, z)
            for key in ("corr", "delta", "x", "y", "rows", "scores"):
                assert torch.equal(one[key][0], batch[key][z]), f"pair {z}: {key}"
            res = sr.run_coarse(emu, ncn, fa[z:z + 1], fb[z:z + 1], k, "cpu")
            off = sr.coarse_ws_offsets(c, ha, wa, hb, wb, k)
            both = _planes(name, mode)[0]["ws"][z]
            for key, nxt in (("fnA", "fnB"), ("fnB", "P")):
                assert torch.equal(res["ws"][0][off[key]:off[nxt]], both[off[key]:off[nxt]]), f"pair {z}: the bytes of {key}"
    finally:
        emu.p2p_ncn_destroy(ncn)
    wc.yardsticks(name, _sd(), mode)                 # magnitudes 1, 2^10, 2^-10 and a dead cell, inside the same bounds
    cm.check_stages(batch, name, _sd(), mode, "emulated ")
    cm.check_rows(batch["rows"], name, _sd(), mode)


def test_channel_limit():
    """1056 (a multiple of 32 past the limit) and 1030 (no multiple of 32) are refused; 1024 is sized."""
    emu = _emu()
    ncn = cm.ncn_create(emu, _sd())
    try:
        for c in (1056, 1030):
            fa = torch.zeros(1, c, 4, 6)
            out = torch.zeros(1, 2, 3, 2, 3)
            ws = torch.zeros(1 << 22, dtype=torch.uint8)
            st = emu.p2p_coarse_forward_batch(emu_lib.ptr(fa), emu_lib.ptr(fa), 1, c, 4, 6, 4, 6, 2, ncn, emu_lib.ptr(out), None,
                                              ctypes.c_void_p((ws.data_ptr() + 255) & ~255), ws.numel() - 256, None)
            assert st == -3, (c, st)                                             # P2P_EUNSUPPORTED
            assert b"1024" in emu.p2p_last_error() and str(c).encode() in emu.p2p_last_error()
        assert emu.p2p_coarse_workspace_bytes(1024, 4, 6, 6, 4, 2) == sr.coarse_ws_offsets(1024, 4, 6, 6, 4, 2)["total"]
    finally:
        emu.p2p_ncn_destroy(ncn)
