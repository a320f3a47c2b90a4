"""ksize = 4 of the coarse stage (4x4x4x4 max-pool with relocalisation on the MFMA accumulators, corr_pool_kernel<4> of
csrc/coarse.hip) executed on the CPU by the test-suite's HIP stand-in (tests/hipemu, see tests/test_kernels_emulated.py):
the reference's own outputs (tests/golden/coarse_*_k4.npz, written by tests/make_golden_k4.py), the oracle on random
shapes, constructed ties, batches, consensus tiles and the argument checks.  Tolerances are those of the k = 2 tests."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import p2p_oracle as orc
from patch2pix_amd.utils import synthetic

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402

K4_CASES = ["coarse_256x320_k4", "coarse_160x352_k4"]


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


@pytest.fixture(scope="module")
def sd():
    return gu.state_dict(0)


@pytest.fixture(scope="module")
def ncn(emu, sd):
    return emu_lib.ncn_create(emu, sd)


def _pack(planes, k):
    return ((planes[0] * k + planes[1]) * k + planes[2]) * k + planes[3]


@pytest.mark.parametrize("name", K4_CASES)
def test_k4_coarse_stage_against_reference_golden(name, emu, ncn):
    g = gu.load(name)
    assert int(g["ksize"]) == 4
    p1, p2 = gu.coarse_inputs(g)
    corr, delta = emu_lib.coarse_forward_batch(emu, ncn, p1[4][None], p2[4][None], 4)
    np.testing.assert_allclose(corr[0].numpy(), g["corr4d"], rtol=2e-4, atol=1e-7)
    ref_code = _pack(g["delta4d"].astype(np.int64), 4).reshape(delta[0].shape)
    assert ref_code.max() > 127, "the fixture does not reach the upper half of the byte"
    assert np.array_equal(delta[0].numpy(), ref_code)
    m, s = emu_lib.coarse_matches_batch(emu, corr, delta, 4, 8)
    assert np.array_equal(m[0].numpy(), g["all_matches"])
    np.testing.assert_allclose(s[0].numpy(), g["all_scores"], rtol=2e-4)


@pytest.mark.parametrize("seed", range(8))
def test_k4_coarse_stage_random_shapes(seed, emu, ncn, sd):
    """Unrelated sizes for the two images (down to one cell), any channel count the library accepts, small batches:
    volume and relocalisation against the oracle, match extraction bit-exact on the kernel's volume."""
    rng = np.random.RandomState(400 + seed)
    ksize = 4
    hA, wA, hB, wB = [int(rng.randint(1, 8)) * ksize for _ in range(4)]
    C, B = int(rng.choice([32, 64, 128, 256])), int(rng.choice([1, 2, 3]))
    g = torch.Generator().manual_seed(40 + seed)
    fa, fb = torch.randn(B, C, hA, wA, generator=g), torch.randn(B, C, hB, wB, generator=g)
    corr, delta = emu_lib.coarse_forward_batch(emu, ncn, fa, fb, ksize)
    m, s = emu_lib.coarse_matches_batch(emu, corr, delta, ksize, 8)
    o_ncn, _, _ = orc.split_params(sd)
    o64, _, _ = orc.split_params(sd, torch.float64)
    for b in range(B):
        rc, rd = orc.coarse_forward(fa[b], fb[b], ksize, o_ncn)
        # the yardstick on ill-conditioned tiny volumes is the fp32 oracle's own distance from an fp64 evaluation
        # (tests/test_kernels_emulated.py::test_coarse_stage_random_shapes)
        r64, _ = orc.coarse_forward(fa[b].double(), fb[b].double(), ksize, o64)
        rel = lambda x: ((x.double() - r64).abs() / r64.abs().clamp_min(1e-30)).max().item()
        print(f"seed {seed} pair {b}: {hA}x{wA} / {hB}x{wB}, C {C}: rel {rel(corr[b]):.3e} (oracle {rel(rc):.3e})")
        assert rel(corr[b]) <= max(3e-4, 4 * rel(rc)), (rel(corr[b]), rel(rc))
        k, d = ksize, delta[b].long()
        assert int((d != _pack(rd, k)).sum()) <= 1, "relocalisation argmax differs beyond a near-tie"
        kd = [d // (k * k * k), (d // (k * k)) % k, (d // k) % k, d % k]
        rm, rs = orc.cal_coarse_matches(corr[b], kd, ksize, 8)
        assert torch.equal(m[b], rm)
        assert torch.allclose(s[b], rs, rtol=1e-4)


def _unit(gen, C):
    v = torch.randn(C, generator=gen)
    return 4.0 * v / v.norm()


@pytest.mark.parametrize("cells", [((0, 0), (0, 0), (0, 1), (0, 1), (1, 0), (1, 0)),      # first tile, first blocks
                                   ((2, 4), (1, 3), (1, 2), (2, 4), (2, 3), (0, 4)),      # last cell = half a 32-row block
                                   ((1, 1), (2, 2), (2, 0), (0, 3), (0, 4), (2, 1))])
def test_k4_ties_take_the_lowest_code(cells, emu, ncn):
    """First maximum in the reference's slice order s = ((di*4+dj)*4+dk)*4+dl (modules.py:13-28): positions with
    bit-identical correlation are built from duplicated feature vectors (equal vectors normalise and multiply to equal
    bits; v and -v on both sides give the same product bits), and a pair of copies of one vector on the two images is
    the cell's maximum (cosine 1).  Feature maps of 12x20 positions = 3x5 cells per image: 240 GEMM rows, i.e. two
    128-row tiles, the second with 112 rows of which the last 16 are half a 32-row block."""
    C, h, w = 64, 12, 20
    gen = torch.Generator().manual_seed(7)
    fa, fb = torch.randn(C, h, w, generator=gen), torch.randn(C, h, w, generator=gen)
    (a1, b1, a2, b2, a3, b3) = cells
    v1, v2, v3 = _unit(gen, C), _unit(gen, C), _unit(gen, C)

    def put(f, cell, d, v):
        f[:, 4 * cell[0] + d[0], 4 * cell[1] + d[1]] = v

    # unique maximum in the last corner: s = 255
    put(fa, a1, (3, 3), v1); put(fb, b1, (3, 3), v1)
    # s = 0 against s = 255 only: the first corner holds v, the last one -v on both images
    put(fa, a2, (0, 0), v2); put(fa, a2, (3, 3), -v2); put(fb, b2, (0, 0), v2); put(fb, b2, (3, 3), -v2)
    # four equal maxima, (di, dj) in {(1, 2), (2, 1)} x (dk, dl) in {(0, 3), (3, 0)}: the lowest is ((1*4+2)*4+0)*4+3 = 99
    put(fa, a3, (1, 2), v3); put(fa, a3, (2, 1), v3); put(fb, b3, (0, 3), v3); put(fb, b3, (3, 0), v3)
    _, delta = emu_lib.coarse_forward_batch(emu, ncn, fa[None], fb[None], 4)
    d = delta[0]
    assert d.dtype == torch.uint8
    got = [int(d[a1[0], a1[1], b1[0], b1[1]]), int(d[a2[0], a2[1], b2[0], b2[1]]), int(d[a3[0], a3[1], b3[0], b3[1]])]
    assert got == [255, 0, 99], got
    # the code 255 survives the unpacking and the match extraction (the relocalised coordinates of that cell)
    corr = torch.zeros((1, 3, 5, 3, 5))
    corr[0, a1[0], a1[1], b1[0], b1[1]] = 5.0
    m, _ = emu_lib.coarse_matches_batch(emu, corr, delta, 4, 8)
    row = m[0][b1[0] * 5 + b1[1]]          # direction B -> A: one row per B cell
    want = [8 * (4 * a1[1] + 3) + 4, 8 * (4 * a1[0] + 3) + 4, 8 * (4 * b1[1] + 3) + 4, 8 * (4 * b1[0] + 3) + 4]
    assert row.tolist() == want, (row.tolist(), want)


def test_k4_coarse_batch_equals_single_pairs(emu, ncn):
    """One launch per kernel for B pairs == B single-pair calls, bit for bit, also when the workspace only holds two
    of the five pairs at a time."""
    pairs = [synthetic.make_correlated_pyramids(520 + i, 96, 128) for i in range(5)]
    fa = torch.stack([p[0][4] for p in pairs])
    fb = torch.stack([p[1][4] for p in pairs])
    singles = [emu_lib.coarse_forward_batch(emu, ncn, fa[i:i + 1], fb[i:i + 1], 4) for i in range(5)]
    for ws_pairs in (5, 2):
        corr, delta = emu_lib.coarse_forward_batch(emu, ncn, fa, fb, 4, ws_pairs=ws_pairs)
        m, s = emu_lib.coarse_matches_batch(emu, corr, delta, 4, 8)
        for i in range(5):
            assert torch.equal(corr[i], singles[i][0][0]) and torch.equal(delta[i], singles[i][1][0])
            m1, s1 = emu_lib.coarse_matches_batch(emu, singles[i][0], singles[i][1], 4, 8)
            assert torch.equal(m[i], m1[0]) and torch.equal(s[i], s1[0])


def test_k4_coarse_stage_is_tile_independent(emu, sd):
    """The consensus kernel's work-group tile must not change a bit of the k = 4 coarse stage either (7x11x7x11 cells:
    last axis not a multiple of 4), forced tiles against the automatic choice and the oracle."""
    p1, p2 = synthetic.make_correlated_pyramids(324, 224, 352)
    o_ncn, _, _ = orc.split_params(sd)
    rc, rd = orc.coarse_forward(p1[4], p2[4], 4, o_ncn)
    ncn = emu_lib.ncn_create(emu, sd)
    base, bdelta = emu_lib.coarse_forward_batch(emu, ncn, p1[4][None], p2[4][None], 4)
    np.testing.assert_allclose(base[0].numpy(), rc.numpy(), rtol=2e-4, atol=1e-7)
    assert int((bdelta[0].long() != _pack(rd, 4)).sum()) <= 1
    for tile in ((2, 3, 2), (0, 2, 5), (30, 6, 6)):
        emu_lib.check(emu, emu.p2p_ncn_set_tile(ncn, *tile), "p2p_ncn_set_tile")
        corr, delta = emu_lib.coarse_forward_batch(emu, ncn, p1[4][None], p2[4][None], 4)
        assert torch.equal(corr, base), f"tile {tile} changes the volume (max |d| {float((corr - base).abs().max()):.3e})"
        assert torch.equal(delta, bdelta)
    emu.p2p_ncn_destroy(ncn)


def test_k4_delta_unpack_full_byte_range(emu):
    """Every code 0..255 through p2p_delta_unpack with ksize 4 (no sign extension of the byte on the way)."""
    codes = torch.arange(256, dtype=torch.uint8)
    out = torch.empty((4, 256), dtype=torch.int64)
    emu_lib.check(emu, emu.p2p_delta_unpack(emu_lib.ptr(codes), 256, 4, emu_lib.ptr(out), None), "p2p_delta_unpack")
    s = torch.arange(256)
    assert torch.equal(out, torch.stack([s // 64, (s // 16) % 4, (s // 4) % 4, s % 4]))


def test_k4_argument_checks(emu, ncn):
    """ksize 3 and every ksize > 4 stay P2P_EUNSUPPORTED (-3); a feature map whose side is not a multiple of 4 is
    P2P_EINVAL (-1) with the library's message."""
    fa = torch.zeros(1, 32, 12, 60)
    out = torch.zeros(1 << 16)
    ws = torch.zeros(1 << 22, dtype=torch.uint8)

    def call(ha, wa, hb, wb, ksize):
        return emu.p2p_coarse_forward_batch(emu_lib.ptr(fa), emu_lib.ptr(fa), 1, 32, ha, wa, hb, wb, ksize, ncn, emu_lib.ptr(out),
                                            None, emu_lib.ptr(ws), ws.numel(), None)

    for ksize in (3, 5, 6, 8):
        assert call(12, 60, 12, 60, ksize) == -3, ksize
        assert b"ksize" in emu.p2p_last_error() and b"1, 2 or 4" in emu.p2p_last_error()
    for sizes in ((6, 8, 8, 8), (8, 8, 8, 6), (8, 10, 8, 8)):
        assert call(*sizes, 4) == -1, sizes
        assert b"multiples of ksize" in emu.p2p_last_error()
    assert call(8, 8, 4, 12, 4) == 0, emu.p2p_last_error()


def test_k4_plain_c_example_end_to_end(emu, ncn, sd, tmp_path):
    """examples/cabi_coarse.c with ksize 4 in its input file, compiled against the stand-in, against the ctypes calls into
    the same emulated library: bit-identical outputs."""
    import subprocess
    import build_emu
    import cabi_example_io as io
    exe = build_emu.build_example()
    pairs = [synthetic.make_correlated_pyramids(720 + i, 96, 128) for i in range(3)]
    fa = torch.stack([p[0][4] for p in pairs]).contiguous()
    fb = torch.stack([p[1][4] for p in pairs]).contiguous()
    io.write_input(tmp_path / "in.bin", sd, fa, fb, 4)
    res = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    corr, delta = emu_lib.coarse_forward_batch(emu, ncn, fa, fb, 4)
    m, sc = emu_lib.coarse_matches_batch(emu, corr, delta, 4, 8)
    c_corr, c_delta, c_m, c_s = io.read_output(tmp_path / "out.bin", corr.numel(), sc.numel(), 4)
    assert np.array_equal(c_corr, corr.numpy().ravel())
    assert np.array_equal(c_delta, delta.numpy().ravel())
    assert np.array_equal(c_m, m.numpy().ravel()) and np.array_equal(c_s, sc.numpy().ravel())
