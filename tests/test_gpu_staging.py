"""The pinned staging ring (patch2pix_amd/staging.py) on the GPU: more stagings in flight than a ring has slots, for
each of the entry points built on it.  Needs an MI355X:  pytest -m gpu"""
import numpy as np
import pytest
import torch

from patch2pix_amd import staging
from patch2pix_amd.utils import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    from patch2pix_amd.utils.eval import model_helper
    return model_helper.load_model(synthetic.make_checkpoint(0), lprint=lambda *a: None)


SIZES = [1 << 10, 1 << 16, 1 << 20]          # bytes, cycled: the buffers of the ring grow in mid-sequence


def test_uploads_outrun_the_ring(dev):
    """20 uploads through 8 slots with nothing between them that waits for the GPU: a slot is only written again when the
    copy that read it has run, and a buffer that is replaced by a larger one stays alive until its copy has."""
    from patch2pix_amd import ops
    rng = np.random.default_rng(1)
    ring = staging.PinnedRing(8)
    sources = [[rng.integers(0, 256, SIZES[i % 3], dtype=np.uint8), torch.from_numpy(rng.integers(-9, 9, (i + 1, 4)))]
               for i in range(20)]
    results = [staging.upload(src, dev, ring) for src in sources]
    small = [rng.integers(-1 << 30, 1 << 30, SIZES[i % 3] // 4).astype(np.int32) if i % 2 == 0 else
             rng.standard_normal((SIZES[i % 3] // 32, 4)) for i in range(20)]
    small_results = [ops.small_to_device(a, torch.int32 if i % 2 == 0 else torch.float64, dev) for i, a in enumerate(small)]
    for (pixels, rows), (got_pixels, got_rows) in zip(sources, results):
        assert got_pixels.device == dev and got_pixels.dtype == torch.uint8 and got_rows.dtype == torch.int64
        assert np.array_equal(got_pixels.cpu().numpy(), pixels) and torch.equal(got_rows.cpu(), rows)
    for a, got in zip(small, small_results):
        assert got.device == dev and tuple(got.shape) == a.shape
        assert np.array_equal(got.cpu().numpy(), a)


def test_readbacks_outrun_the_ring(dev):
    ring = staging.PinnedRing(4)
    g = torch.Generator(device=dev).manual_seed(2)
    tensors = [torch.randn((257, 9), generator=g, device=dev) for _ in range(ring.slots + 1)]
    handles = [staging.readback([t], ring) for t in tensors]
    assert handles[0].stale and handles[0].wait() is None
    for t, h in zip(tensors[1:], handles[1:]):
        assert not h.stale
        view, = h.wait()
        assert view.is_pinned() and view.dtype == torch.float32
        assert torch.equal(view, t.cpu())


def _as_batch(image, dev):
    return ((torch.from_numpy(image).permute(2, 0, 1).float() / 255.0 - 0.45) / 0.225)[None].to(dev)


def _assert_same_matches(got, want):
    """The comparison of test_gpu_parity.py::test_stream_equals_per_pair_calls on (fine, scores, coarse) of one pair: rows
    are matched by their coarse match."""
    (m, _, c), (rm, _, rc) = [[t.cpu().numpy() for t in triple] for triple in (got, want)]
    ref = {tuple(np.round(r, 6)): i for i, r in enumerate(rc)}
    hits = [(i, ref[tuple(np.round(r, 6))]) for i, r in enumerate(c) if tuple(np.round(r, 6)) in ref]
    assert len(hits) >= 0.9 * max(len(rc), 1), (len(hits), len(rc))
    if hits:
        gi = np.array([h[0] for h in hits]); ri = np.array([h[1] for h in hits])
        assert np.median(np.abs(m[gi] - rm[ri]).max(axis=1)) < 0.02


def test_ticket_take_over(net, dev):
    """Five tickets issued before any is consumed: the fifth takes the staging slot of the first, which then copies its
    match arrays itself -- and every ticket still gives what the one-at-a-time call gives."""
    with torch.no_grad():
        feats = [net._pyramids(*[_as_batch(im, dev) for im in synthetic.make_image_pair(40 + i, 96, 128)]) for i in range(5)]
        tickets = [net.coarse_async(f1, f2, ksize=2) for f1, f2 in feats]
        assert [t["staged"].stale for t in tickets] == [True, False, False, False, False]
        results = [net.fine_from_ticket(t) for t in tickets]
        for (f1, f2), (fine, scores, coarse) in zip(feats, results):
            want = net.predict_fine_from_feats(f1, f2, ksize=2)
            assert len(fine) == 1 and fine[0].shape[0] > 0
            _assert_same_matches((fine[0], scores[0], coarse[0]), [w[0] for w in want])


def test_filter_coarse_uploads_outrun_the_ring(dev):
    from patch2pix_amd.networks.utils import filter_coarse
    g = torch.Generator().manual_seed(4)
    cases = []
    for _ in range(10):
        rows = torch.randint(0, 1 << 15, (1000, 4), generator=g)
        rows[500:900] = rows[:400]                      # mutual matches: rows that occur twice
        cases.append((rows[None], torch.rand((1, 1000), generator=g)))
    got = [filter_coarse(rows.to(dev), scores.to(dev), 0.5, True) for rows, scores in cases]
    for (rows, scores), (got_rows, got_scores) in zip(cases, got):
        want_rows, want_scores = filter_coarse(rows, scores, 0.5, True)
        assert got_rows[0].device == dev and 0 < want_rows[0].shape[0] < 1000
        assert torch.equal(got_rows[0].cpu(), want_rows[0]) and torch.equal(got_scores[0].cpu(), want_scores[0])


def test_device_keying(dev):
    ring = staging.PinnedRing(2)
    first = ring.take(torch.device("cuda"), 16)
    second = ring.take(torch.device("cuda", torch.cuda.current_device()), 16)
    third = ring.take(torch.device("cuda"), 16)
    assert second is not first and third is first          # one ring: the second take got the slot after the first
    assert first.device == second.device == torch.device("cuda", torch.cuda.current_device())
