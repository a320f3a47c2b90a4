"""The reference's `networks.ncn.extract_ncmatches` on the match kernels of the coarse stage (p2p_coarse_matches_topk_batch with
upsample 1 and no centring; the half of the requested direction is returned)."""
import numpy as np
import torch

from ... import ops

MAX_TOPK = 8


def _pack_delta(delta4d, ksize, shape):
    """The reference's four int64 tensors [B,1,h1,w1,h2,w2] -> the packed byte s = ((i k + j) k + k') k + l."""
    if delta4d is None:
        return None
    if not 1 <= ksize <= 4:
        raise NotImplementedError(f"ksize {ksize}: relocalisation codes must fit a byte (ksize 1 to 4)")
    di, dj, dk, dl = [d.reshape(shape).to(torch.int64) for d in delta4d]
    return (((di * ksize + dj) * ksize + dk) * ksize + dl).to(torch.uint8)


def _extract(corr4d, delta4d, topk, ksize, do_softmax, invert):
    """-> (jA, iA, jB, iB, score), each [B, n * topk] in the reference's order."""
    if not corr4d.is_cuda:
        raise RuntimeError(f"corr4d must be on the GPU (got {corr4d.device}): the operators have no CPU path")
    if corr4d.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("corr4d requires grad: the operators are inference only (wrap the call in torch.no_grad())")
    if topk > MAX_TOPK:
        raise NotImplementedError(f"topk {topk}: at most {MAX_TOPK} candidates per cell are implemented")
    b, ch, fs1, fs2, fs3, fs4 = corr4d.size()
    x = corr4d.detach().reshape(b, fs1, fs2, fs3, fs4)
    delta = _pack_delta(delta4d, ksize, x.shape)
    m, s = ops.coarse_matches_topk_batch(x, delta, ksize if delta is not None else 1, 1, False, topk, do_softmax)
    nb = topk * fs3 * fs4
    m, s = (m[:, nb:], s[:, nb:]) if invert else (m[:, :nb], s[:, :nb])
    return m[..., 0].contiguous(), m[..., 1].contiguous(), m[..., 2].contiguous(), m[..., 3].contiguous(), s.contiguous()


def corr_to_matches(corr4d, delta4d=None, ksize=1, do_softmax=True, scale='positive', invert_matching_direction=False,
                    return_indices=True):
    """Reference extract_ncmatches.py:6-94."""
    jA, iA, jB, iB, score = _extract(corr4d, delta4d, 1, ksize, do_softmax, invert_matching_direction)
    if return_indices:
        return (jA, iA, jB, iB, score)
    b, ch, fs1, fs2, fs3, fs4 = corr4d.size()
    lo = {'centered': -1, 'positive': 0}[scale]
    # the float32 of np.linspace at the indices: what indexing the reference's FloatTensor meshgrids gives
    axis = lambda n: torch.from_numpy(np.linspace(lo, 1, n * ksize).astype(np.float32)).to(corr4d.device)
    return (axis(fs2)[jA], axis(fs1)[iA], axis(fs4)[jB], axis(fs3)[iB], score)


def corr_to_matches_topk(corr4d, delta4d=None, topk=1, ksize=1, do_softmax=True, invert_matching_direction=False):
    """Reference extract_ncmatches.py:96-158; equal values are ranked by ascending cell index (include/p2p_hip.h)."""
    return _extract(corr4d, delta4d, int(topk), ksize, do_softmax, invert_matching_direction)
