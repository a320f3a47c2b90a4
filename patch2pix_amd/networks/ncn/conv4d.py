"""The reference's `networks.ncn.conv4d` on the HIP Conv4d layer (p2p_conv4d_*): exact fp32 on the matrix cores, inference only."""
import math

import torch
from torch.nn import Module
from torch.nn.parameter import Parameter

from ... import ops

def _packed(owner, filters_stored, bias, device, source):
    """The packed layer of a MODULE's `source` parameters (which the module keeps alive), rebuilt when one of them changed
    (identity, version counter, storage)."""
    sig = (str(device),) + ops.tensor_signature([t for t in source if t is not None])
    hit = owner.get("conv")
    if hit is None or hit[0] != sig:
        owner["conv"] = hit = (sig, ops.Conv4dWeights(filters_stored, bias, device))
    return hit[1]


def conv4d(data, filters, bias=None, permute_filters=True, use_half=False):
    """Reference conv4d.py:12-74.  filters: [c_out, c_in, k, k, k, k] with permute_filters, else the stored layout
    [k, c_out, c_in, k, k, k].  The filters are packed and uploaded on every call: nothing keeps a caller's tensors alive, so
    nothing could tell a new tensor from a freed one at the same address.  A layer that is applied repeatedly belongs in a
    `Conv4d` module, which packs once per parameter version."""
    if use_half:
        raise NotImplementedError("conv4d(use_half=True): the layer runs in exact fp32 only")
    if not data.is_cuda:
        raise RuntimeError(f"data must be on the GPU (got {data.device}): the operators have no CPU path")
    stored = filters.detach().permute(2, 0, 1, 3, 4, 5) if permute_filters else filters.detach()
    return ops.conv4d_forward_batch(data, ops.Conv4dWeights(stored, bias, data.device))


class Conv4d(Module):
    """Reference conv4d.py:77-130 (a _ConvNd of stride 1 without padding argument): `weight` is kept in the stored layout
    [k, c_out, c_in, k, k, k] when pre_permuted_filters (the default), `bias` [c_out] or None.  A reference state_dict loads
    strictly."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, pre_permuted_filters=True):
        super().__init__()
        k = int(kernel_size)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, (k,) * 4
        self.pre_permuted_filters = pre_permuted_filters
        self.use_half = False
        weight = torch.empty(out_channels, in_channels, k, k, k, k)
        # _ConvNd.reset_parameters on the [c_out, c_in, k, k, k, k] tensor, before the permutation
        torch.nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_channels * k ** 4)
            self.bias = Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)
        self.weight = Parameter(weight.permute(2, 0, 1, 3, 4, 5).contiguous() if pre_permuted_filters else weight)
        self._hip = {}

    def __getstate__(self):      # copies and pickles do not share the device handle
        state = self.__dict__.copy()
        state["_hip"] = {}
        return state

    def forward(self, input):
        if self.use_half:
            raise NotImplementedError("Conv4d.use_half: the layer runs in exact fp32 only")
        if not input.is_cuda:
            raise RuntimeError(f"input must be on the GPU (got {input.device}): the operators have no CPU path")
        stored = self.weight.detach() if self.pre_permuted_filters else self.weight.detach().permute(2, 0, 1, 3, 4, 5)
        return ops.conv4d_forward_batch(input, _packed(self._hip, stored, self.bias, input.device, (self.weight, self.bias)))
