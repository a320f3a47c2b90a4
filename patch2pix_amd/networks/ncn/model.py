"""The reference's `networks.ncn.model` (the operators Patch2Pix builds on; the legacy ImMatchNet classes are out of scope) on the
HIP kernels: inference only, float32 tensors on the GPU."""
import torch
import torch.nn as nn

from ... import ops
from .conv4d import Conv4d


def MutualMatching(corr4d):
    """Reference ncn/model.py:157-176: corr4d [B,1,hA,wA,hB,wB] -> the same shape."""
    if corr4d.dim() != 6 or corr4d.shape[1] != 1:
        raise ValueError(f"MutualMatching expects [B,1,hA,wA,hB,wB], got {tuple(corr4d.shape)}")
    return ops.mutual_matching_batch(corr4d[:, 0]).unsqueeze(1)


class NeighConsensus(torch.nn.Module):
    """Reference ncn/model.py:124-155.  Parameters conv.{2i}.weight / .bias in the stored layout, so a reference state_dict loads
    strictly.  The released stack ([3,3] / [16,1], symmetric) runs the tuned kernel, every other stack within ops.ncn_layout's
    limits the generic handle; a stack outside them raises what ops.ncn_layout raises, at construction."""

    def __init__(self, use_cuda=True, kernel_sizes=[3, 3, 3], channels=[10, 10, 1], symmetric_mode=True):
        super().__init__()
        self.layout = ops.ncn_layout(dict(kernel_sizes=kernel_sizes, channels=channels), symmetric_mode)
        self.symmetric_mode = symmetric_mode
        self.kernel_sizes = kernel_sizes
        self.channels = channels
        nn_modules = []
        for i, (k_size, ch_out) in enumerate(zip(kernel_sizes, channels)):
            ch_in = 1 if i == 0 else channels[i - 1]
            nn_modules.append(Conv4d(in_channels=ch_in, out_channels=ch_out, kernel_size=k_size, bias=True))
            nn_modules.append(nn.ReLU(inplace=True))
        self.conv = nn.Sequential(*nn_modules)
        self._hip_sig = self._hip = None
        if use_cuda:
            self.conv.cuda()

    def __getstate__(self):      # copies and pickles do not share the device handle
        state = self.__dict__.copy()
        state["_hip"] = state["_hip_sig"] = None
        return state

    def _weights(self, device):
        """The packed handle, rebuilt when a parameter changed (identity, version counter, storage) or the device did.  Like
        ResNet34._hip_signature it cannot see an edit through `param.data` (`param.data.copy_()`, `param.data.mul_()`): that
        keeps identity and storage and does not advance the parameter's version counter.  Use load_state_dict or an in-place
        operation on the parameter itself (under torch.no_grad())."""
        sd = {}
        for i in range(len(self.kernel_sizes)):
            layer = self.conv._modules[str(2 * i)]
            sd[f"conv.{2 * i}.weight"], sd[f"conv.{2 * i}.bias"] = layer.weight, layer.bias
        sig = (str(device),) + ops.tensor_signature(sd.values())
        if self._hip_sig != sig:
            self._hip = ops.NcnWeights.from_state_dict({k: v.detach() for k, v in sd.items()}, device, self.symmetric_mode)
            self._hip_sig = sig
        return self._hip

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"x must be on the GPU (got {x.device}): the operators have no CPU path")
        if x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("x requires grad: the operators are inference only (wrap the call in torch.no_grad())")
        if x.dim() != 6 or x.shape[1] != 1:
            raise ValueError(f"NeighConsensus expects [B,1,hA,wA,hB,wB], got {tuple(x.shape)}")
        return ops.neigh_consensus_batch(x.detach()[:, 0], self._weights(x.device)).unsqueeze(1)
