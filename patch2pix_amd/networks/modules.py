"""The reference's `networks.modules` (matching operators) on the HIP kernels of libp2p_hip.so: the same names, signatures and
defaults; inference only, float32 tensors on the GPU, no CPU path.  Launches go to the current stream of the input's device."""
import torch

from .. import ops

_FEAT_REGRESS_NET = ("FeatRegressNet is not provided as a module: it takes materialised patches, and the fine stage stays fused "
                     "(networks.patch2pix.Patch2Pix runs it inside p2p_regress*)")


def L2Normalize(feat, dim):
    """feat / sqrt(sum(feat^2, dim) + 1e-6) (reference modules.py:6)."""
    return ops.l2_normalize(feat, dim)


def cal_conv_out_size(w, kernel_size, stride, padding):
    return (w - kernel_size + 2 * padding) // stride + 1


def maxpool4d(corr4d_hres, k_size=4):
    """Reference modules.py:11-34: corr4d_hres [B,1,H1,W1,H2,W2] -> (corr4d [B,1,H1/k,...], max_i, max_j, max_k, max_l), the four
    int64 tensors of the same shape with the position of the first maximum inside each k^4 window."""
    if corr4d_hres.dim() != 6 or corr4d_hres.shape[1] != 1:
        raise ValueError(f"maxpool4d expects [B,1,H1,W1,H2,W2], got {tuple(corr4d_hres.shape)}")
    pooled, delta = ops.maxpool4d_batch(corr4d_hres[:, 0], k_size)
    mi, mj, mk, ml = ops.delta_unpack(delta, int(k_size))
    return (pooled.unsqueeze(1), mi.unsqueeze(1), mj.unsqueeze(1), mk.unsqueeze(1), ml.unsqueeze(1))


class FeatCorrelation(torch.nn.Module):
    """Reference modules.py:36-53: the plain feature product, '4D' -> [b,1,h1,w1,h2,w2], '3D' -> [b,h2*w2,h1,w1]."""

    def __init__(self, shape='4D'):
        super().__init__()
        self.shape = shape

    def forward(self, feat1, feat2):
        b, c, h1, w1 = feat1.size()
        b, c, h2, w2 = feat2.size()
        correlation = ops.correlation_batch(feat1, feat2)
        if self.shape == '3D':
            correlation = correlation.view(b, h1, w1, h2 * w2).permute(0, 3, 1, 2)
        elif self.shape == '4D':
            correlation = correlation.view(b, h1, w1, h2, w2).unsqueeze(1)
        return correlation


def __getattr__(name):
    if name == "FeatRegressNet":
        raise NotImplementedError(_FEAT_REGRESS_NET)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
