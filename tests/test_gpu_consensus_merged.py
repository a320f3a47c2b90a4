"""The fused consensus kernel (csrc/consensus.hip) as one work-group of eight waves per tile that owns BOTH branches: waves
0-3 the direct branch, waves 4-7 the transposed one, the input planes staged once for the two.  Needs an MI355X:  pytest -m gpu

What the merge could break, at the smallest shapes that cross each seam: the b tiles (a halo crossing, a partial last tile,
a single partly filled one) with the automatic tile and with forced tb = 8 and tb = 10, the fixed-tile instantiations (tb = 5
and 10), the two halves on an input with X != X^T (a swapped or doubled half), both output forms (two arrays | both branches
added into one zeroed array), and the independence of a pair's bits from the tile and the batch.  Bar against the oracle:
that of test_gpu_parity.py::test_fused_consensus_vs_oracle (3e-6 of the largest reference value); everything else bit for bit.
"""
import ctypes

import pytest
import torch

import golden_util as gu
import stage_reference as sr
from oracle import p2p_oracle as orc

pytestmark = pytest.mark.gpu

REL_TOL = 3e-6          # test_fused_consensus_vs_oracle


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from patch2pix_amd import ops
    return ops


@pytest.fixture(scope="module")
def sd():
    return gu.state_dict(0)


@pytest.fixture()
def ncn(dev, ops, sd):
    """A handle of its own per test: a forced tile stays with the handle."""
    return ops.NcnWeights(sd["ncn.conv.0.weight"], sd["ncn.conv.0.bias"], sd["ncn.conv.2.weight"], sd["ncn.conv.2.bias"], dev)


def _volume(pairs, dims, seed):
    """Seeded, X != X^T; the last item of a batch with negative values far above 1 (rescaled inside the kernel)."""
    x = torch.rand(pairs, *dims, generator=torch.Generator().manual_seed(seed))
    if pairs > 1:
        x[-1] = (x[-1] - 0.5) * 300.0
    return x


_refs = {}


def _branches(x, sd):
    """Oracle, branch by branch (oracle/p2p_oracle.py neigh_consensus is their sum); computed once per input."""
    key = (tuple(x.shape), float(x.double().sum()))
    if key not in _refs:
        o = orc.split_params(sd)[0]
        net = lambda v: torch.relu(orc.conv4d(torch.relu(orc.conv4d(v, o["w1"], o["b1"])), o["w2"], o["b2"]))
        y1 = net(x.unsqueeze(0))[0]
        y2 = net(x.permute(2, 3, 0, 1).contiguous().unsqueeze(0))[0].permute(2, 3, 0, 1)
        assert torch.equal(y1 + y2, orc.neigh_consensus(x, o))
        _refs[key] = (y1, y2)
    return _refs[key]


def _check_sum(y, x, sd, what):
    for b in range(x.shape[0]):
        y1, y2 = _branches(x[b], sd)
        ref = y1 + y2
        err, bar = float((y[b] - ref).abs().max()), REL_TOL * float(ref.abs().max())
        print(f"consensus[{what}] item {b}: max |d| {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, b)


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("d1", [16, 9, 5])
def test_b_tile_seams(d1, pairs, dev, ops, ncn, sd):
    """d1 = 16 (b-halo crossings), 9 (a partial last b tile), 5 (a single, partly filled b tile), each 3 x d1 x 9 x 12: the
    runtime-valued body.  The automatic tile, then tb = 8 and tb = 10 forced: all against the oracle through the first, bit
    for bit among themselves and against a second call."""
    dims = (3, d1, 9, 12)
    x = _volume(pairs, dims, 100 * d1 + pairs)
    xd = x.to(dev)
    y = ops.neigh_consensus_batch(xd, ncn).cpu()
    _check_sum(y, x, sd, f"{dims} x {pairs}")
    assert torch.equal(ops.neigh_consensus_batch(xd, ncn).cpu(), y), "a second call gives other bits"
    for tile in ((0, 8, 8), (0, 10, 8), (2, 8, 4)):
        ncn.set_tile(*tile)
        assert torch.equal(ops.neigh_consensus_batch(xd, ncn).cpu(), y), tile


@pytest.mark.parametrize("d0", [1, 3])
def test_fixed_tile_instantiations(d0, dev, ops, ncn, sd):
    """(d1, d2, d3) = (12, 9, 40) selects the compile-time tile (tc, td, P) = (8, 40, 44); d0 = 1 is the shortest march there
    is.  tb = 5 (what a launch this small picks) and tb = 10 (the tile of the benched batches; 12 = one whole and one partial b
    tile, 9 = one whole and one partial c tile), and a runtime-valued tile: the same bits."""
    dims = (d0, 12, 9, 40)
    x = _volume(1, dims, 7 + d0)
    xd = x.to(dev)
    y = ops.neigh_consensus_batch(xd, ncn).cpu()
    _check_sum(y, x, sd, f"{dims}")
    for tile in ((0, 5, 8), (0, 10, 8), (0, 8, 8), (0, 10, 6)):
        ncn.set_tile(*tile)
        got = ops.neigh_consensus_batch(xd, ncn).cpu()
        assert torch.equal(got, y), tile
        assert torch.equal(ops.neigh_consensus_batch(xd, ncn).cpu(), got), ("second call", tile)


def _coarse_two_arrays(fa, fb, ncn, ops):
    """p2p_coarse_forward_batch at ksize 1 on a workspace of this test's own -> per pair (X, Y, Y2): the consensus kernel's
    input (the mutual-matched correlations) and its two-array output form, read back from the pair's workspace block."""
    _lib = ops._lib
    nb, c, ha, wa = fa.shape
    hb, wb = fb.shape[2:]
    per = _lib.p2p_coarse_workspace_bytes_for(ncn.handle, c, ha, wa, hb, wb, 1)
    off = sr.coarse_ws_offsets(c, ha, wa, hb, wb, 1)
    assert per == off["total"]
    ws = torch.zeros(nb * per, dtype=torch.uint8, device=fa.device)
    corr = torch.empty(nb, ha, wa, hb, wb, dtype=torch.float32, device=fa.device)
    with torch.cuda.device(fa.device):
        _lib.check(_lib.p2p_coarse_forward_batch(fa.data_ptr(), fb.data_ptr(), nb, c, ha, wa, hb, wb, 1, ncn.handle, corr.data_ptr(),
                                                 None, ws.data_ptr(), ws.numel(), ops._stream()), "p2p_coarse_forward_batch")
    torch.cuda.synchronize()
    cells = ha * wa * hb * wb
    part = lambda b, name: ws[b * per + off[name]:b * per + off[name] + 4 * cells].view(torch.float32).view(ha, wa, hb, wb).clone()
    return [tuple(part(b, n) for n in ("P", "Y", "Y2")) for b in range(nb)]


def test_both_output_forms_on_an_asymmetric_volume(dev, ops, ncn, sd):
    """3 x 16 x 4 x 10 (d0 d1 != d2 d3, X != X^T: the branches differ), three pairs.  Two-array form (the coarse stage): each
    array against ITS branch of the oracle -- a swapped or doubled half fails here; the add-into-one form (the operator) on the
    same X equals Y + Y2 bit for bit; a pair alone gives the bits it has inside the batch, in both forms."""
    g = torch.Generator().manual_seed(31)
    fa, fb = torch.randn(3, 32, 3, 16, generator=g).to(dev), torch.randn(3, 32, 4, 10, generator=g).to(dev)
    for tile in ((0, 0, 0), (0, 10, 8), (0, 8, 8)):
        ncn.set_tile(*tile)
        trip = _coarse_two_arrays(fa, fb, ncn, ops)
        x = torch.stack([t[0] for t in trip])
        added = ops.neigh_consensus_batch(x, ncn)
        for b, (xb, y, y2) in enumerate(trip):
            r1, r2 = _branches(xb.cpu(), sd)
            bar = REL_TOL * float((r1 + r2).abs().max())
            e1, e2 = float((y.cpu() - r1).abs().max()), float((y2.cpu() - r2).abs().max())
            print(f"consensus[two arrays, tile {tile}] pair {b}: max |d| direct {e1:.3e}, transposed {e2:.3e}, bar {bar:.3e}; "
                  f"max |direct - transposed| of the oracle {float((r1 - r2).abs().max()):.3e}")
            assert float((r1 - r2).abs().max()) > 100 * bar, "the input does not tell the branches apart"
            assert e1 <= bar and e2 <= bar, (tile, b)
            assert torch.equal(added[b], y + y2), (tile, b)
            assert torch.equal(ops.neigh_consensus_batch(xb[None], ncn)[0], added[b]), ("alone", tile, b)
        alone = _coarse_two_arrays(fa[1:2], fb[1:2], ncn, ops)[0]
        assert all(torch.equal(p, q) for p, q in zip(alone, trip[1])), ("alone, two arrays", tile)
        if tile == (0, 0, 0):
            base = trip
        else:
            assert all(torch.equal(p, q) for tb_, t0 in zip(trip, base) for p, q in zip(tb_, t0)), tile
