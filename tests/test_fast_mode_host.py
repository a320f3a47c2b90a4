"""Mode 'fp16' (P2P_REGRESS_FP16), host side: the ABI (mode id, workspace query, refusals), the Python names, and the packed
weight streams -- ONE fp16 plane per operand, half the bytes of the 'fp16x2w' streams, every stored operand the fp16 rounding
of the scaled weight.  The packers are the library's own host code, called in the CPU build of tests/hipemu (the handle keeps
its streams private; the packers are what fills them)."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

import emu_lib  # noqa: E402
import fast_mode_reference as fm  # noqa: E402
import golden_util as gu  # noqa: E402
import regressor_reference as rg  # noqa: E402
from patch2pix_amd import _lib as real  # noqa: E402

S1_UNITS, S2_WINO_BLOCKS, XPF = 2 * (4 + 9 * 2 * 16), 16 * 4 * 16, 8
WH1_HALVES_2 = 8 * (S1_UNITS + XPF) * 1024          # fp16 elements of conv1's two-plane stream
WW2_HALVES_2 = S2_WINO_BLOCKS * 8192                # ... of the two-plane Winograd filter blocks


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def test_names_and_version():
    assert real.p2p_version() & ~real.VERSION_EXPERIMENT >= 111
    assert real.REGRESS_MODES_LOSSY == {"fp16": fm.MODE_ID}
    assert fm.MODE_ID not in real.REGRESS_MODES.values() and fm.MODE_ID != real.REGRESS_GENERIC
    assert real.REGRESS_MODES == {"f32": 0, "fp16x2": 3, "fp16x2w": 4}       # the dict existing tests iterate over is as it was


def test_set_mode_on_tuned_and_generic_handles(emu):
    sd = gu.state_dict(0)
    h, keep = fm.create(emu, fm.sub_sd(sd, "regress_mid."), real.REGRESS_MODES["fp16x2w"])
    try:
        assert emu.p2p_regressor_get_mode(h) == 4                       # the default stays fp16x2w
        assert emu.p2p_regressor_set_mode(h, fm.MODE_ID) == 0
        assert emu.p2p_regressor_get_mode(h) == fm.MODE_ID
        assert emu.p2p_regress_workspace_bytes_for(h, 9) == emu.p2p_regress_workspace_bytes_mode(9, fm.MODE_ID)
        assert emu.p2p_regressor_set_mode(h, 4) == 0 and emu.p2p_regressor_set_mode(h, fm.MODE_ID) == 0     # and back again
    finally:
        emu.p2p_regressor_destroy(h)
    case = "B"                                                          # the smallest generic configuration
    st, g = rg.create_config(emu, rg.case_params(case)[0], rg.CASES[case])
    assert st == 0
    try:
        assert emu.p2p_regressor_set_mode(g, fm.MODE_ID) == -3          # P2P_EUNSUPPORTED, like f32
        assert emu.p2p_regressor_set_mode(g, 0) == -3
    finally:
        emu.p2p_regressor_destroy(g)


@pytest.mark.parametrize("lib_name", ["real", "emu"])
def test_workspace_query(lib_name, emu):
    lib = real.lib if lib_name == "real" else emu
    lib.p2p_regress_workspace_bytes_mode.restype = ctypes.c_size_t
    lib.p2p_regress_workspace_bytes.restype = ctypes.c_size_t
    for n in (1, 8, 4000):
        got = lib.p2p_regress_workspace_bytes_mode(n, fm.MODE_ID)
        assert 0 < got <= lib.p2p_regress_workspace_bytes_mode(n, 4), n
        assert lib.p2p_regress_workspace_bytes(n) == lib.p2p_regress_workspace_bytes_mode(n, 4), n     # unchanged: the default mode's
    # the carve-up of fp16x2w with half the bytes per block of the transformed input
    n = 9
    base = lib.p2p_regress_workspace_bytes_mode(n, 3)
    u2 = lib.p2p_regress_workspace_bytes_mode(n, 4)
    u1 = lib.p2p_regress_workspace_bytes_mode(n, fm.MODE_ID)
    rows = 16
    assert u2 - u1 == 16 * (rows // 8) * 16 * 8192 and u1 > base


def _pack(emu, sd):
    """Both packers of both passes on the mid regressor -> dict of int16 views of the streams + the exponents."""
    c1 = sd["regress_mid.conv.0.weight"].float().contiguous()
    c2 = sd["regress_mid.conv.2.weight"].float().contiguous()
    out = {}
    # the packers are C++ symbols of the library (regress_common.h), reached by their Itanium-mangled names:
    #   void p2p::pack_h2_weights(const float *conv1_w, const float *conv2_w, float *wh1, float *wh2, int *t1, int *t2)
    #   void p2p::pack_wino_weights(const float *conv2_w, float *ww2, int *t2)
    # and the same two in p2p::fp16x1 (the nested name shifts the substitution indices S1_.. -> S2_..)
    def symbol(name):
        fn = getattr(emu, name, None)
        assert fn is not None, f"{name} is not exported: did the prototype of a weight packer in regress_common.h change?"
        return fn
    for tag, ns, halves1, halves2 in (("two", "", WH1_HALVES_2, WW2_HALVES_2), ("one", "6fp16x1", WH1_HALVES_2 // 2, WW2_HALVES_2 // 2)):
        ph2 = symbol(f"_ZN3p2p{ns}15pack_h2_weightsEPKfS{'2' if ns else '1'}_PfS{'3' if ns else '2'}_PiS{'4' if ns else '3'}_")
        pw = symbol(f"_ZN3p2p{ns}17pack_wino_weightsEPKfPfPi")
        ph2.restype = pw.restype = None
        ph2.argtypes = [ctypes.c_void_p] * 6
        pw.argtypes = [ctypes.c_void_p] * 3
        w1 = torch.zeros(halves1, dtype=torch.int16)
        w2 = torch.zeros(halves2, dtype=torch.int16)
        t1, t2 = torch.zeros(512, dtype=torch.int32), torch.zeros(512, dtype=torch.int32)
        ph2(c1.data_ptr(), None, w1.data_ptr(), None, t1.data_ptr(), None)
        pw(c2.data_ptr(), w2.data_ptr(), t2.data_ptr())
        out[tag] = (w1, w2, t1, t2)
    return c1, c2, out


def test_streams_are_one_rounded_plane_of_half_the_bytes(emu):
    c1, c2, packed = _pack(emu, gu.state_dict(0))
    (a1, a2, t1a, t2a), (b1, b2, t1b, t2b) = packed["two"], packed["one"]
    assert b1.numel() * 2 == a1.numel() and b2.numel() * 2 == a2.numel()          # half the bytes
    assert torch.equal(t1a, t1b) and torch.equal(t2a, t2b)                        # the same exact power-of-two scales
    # conv1: a single-plane unit [lane 64][8] is the FIRST plane of the two-plane unit [plane 2][lane 64][8] at the same
    # stream position (that layout is pinned by the existing tests of the two-plane stream) ...
    assert torch.equal(b1.view(-1, 512), a1.view(-1, 2, 512)[:, 0])
    # ... and holds, per wave (64 output channels), exactly the fp16 roundings of the scaled fp32 weights (and zero padding)
    for w in range(8):
        rows = slice(64 * w, 64 * w + 64)
        want = torch.ldexp(c1[rows].double(), t1b[rows].view(-1, 1, 1, 1)).float().half().view(torch.int16).flatten()
        got = b1.view(8, -1)[w]
        want, got = want[want != 0].sort().values, got[(got != 0) & (got != -32768)].sort().values
        want = want[want != -32768]
        assert torch.equal(want, got), f"wave {w}"
    # conv2: the transformed filters, computed in fp64 and rounded ONCE to fp16: block [position][column block][K chunk]
    # of [column 128][4 pieces of 8 K, XOR-swizzled by (column >> 2) & 3]
    wt = fm.transformed_filters(c2.double())                                      # [n, k, i, j]
    ref = torch.ldexp(wt, t2b.view(-1, 1, 1, 1)).float().half().view(torch.int16)
    blk = b2.view(16, 4, 16, 128, 4, 8)                                           # p, nb, kc, col, slot, e
    col = torch.arange(128)
    for q in range(4):
        slot = q ^ ((col >> 2) & 3)
        got = blk[:, :, :, col, slot, :]                                          # [p, nb, kc, col, e]: k = 32 kc + 8 q + e
        want = ref.view(4, 128, 16, 4, 8, 16)[:, :, :, q].permute(4, 0, 2, 1, 3)  # n = 128 nb + col; -> [p, nb, kc, col, e]
        assert torch.equal(got, want), f"piece {q}"
    # the first plane of the two-plane blocks is the same rounding
    assert torch.equal(a2.view(-1, 2, 4096)[:, 0], b2.view(-1, 4096))
