"""Generic consensus stacks without a GPU: ops.ncn_layout (inference from a state_dict, validation), the argument errors of
p2p_ncn_create_config and of the workspace queries (validated before the device is touched), the torch restatement of
tests/ncn_reference.py against the reference's goldens, and the parameter holder Patch2Pix builds for a non-released stack."""
import ctypes
from argparse import Namespace

import pytest
import torch

import ncn_reference as nr
from patch2pix_amd import ops


def test_layout_is_read_from_a_state_dict():
    for case, lay in nr.CASES.items():
        got = ops.ncn_layout(nr.weights(case))
        assert got == dict(lay, symmetric_mode=True), case               # a state_dict does not say: the default
        assert ops.ncn_layout(nr.weights(case), symmetric_mode=lay["symmetric_mode"]) == lay
    assert ops.ncn_layout(None) == ops.RELEASED_NCN_LAYOUT == nr.CASES["R"]
    assert ops.ncn_layout(Namespace(kernel_sizes=(5, 3), channels=(7, 1), symmetric_mode=False)) == nr.CASES["M"]
    assert ops.ncn_layout(dict(kernel_sizes=[3], channels=[1])) == nr.CASES["S"]
    assert ops.ncn_shapes(nr.CASES["P"]) == {k: tuple(v.shape) for k, v in nr.weights("P").items()}


def test_layout_validation():
    for bad in (dict(kernel_sizes=[7, 3], channels=[16, 1]), dict(kernel_sizes=[3, 3], channels=[17, 1]),
                dict(kernel_sizes=[3] * 5, channels=[4, 4, 4, 4, 1]), dict(kernel_sizes=[3, 3], channels=[16, 2])):
        with pytest.raises(NotImplementedError):
            ops.ncn_layout(bad)
    for bad in (dict(kernel_sizes=[3, 3], channels=[16]), dict(kernel_sizes=[], channels=[]), dict(kernel_sizes=[3, 0], channels=[4, 1]),
                dict(channels=[1])):
        with pytest.raises(ValueError):
            ops.ncn_layout(bad)
    sd = nr.weights("N")
    broken = dict(sd, **{"conv.2.weight": torch.zeros(3, 10, 9, 3, 3, 3)})          # channel chain broken
    with pytest.raises(ValueError, match="input channels"):
        ops.ncn_layout(broken)
    with pytest.raises(ValueError, match="stored layout"):
        ops.ncn_layout(dict(sd, **{"conv.0.weight": torch.zeros(3, 10, 1, 3, 5, 3)}))   # not cubic
    with pytest.raises(ValueError, match="input channels"):
        ops.ncn_layout(dict(sd, **{"conv.0.weight": torch.zeros(3, 10, 2, 3, 3, 3)}))   # first c_in != 1
    with pytest.raises(ValueError, match="bias"):
        ops.ncn_layout({k: v for k, v in sd.items() if k != "conv.4.bias"})


def test_constructor_keeps_its_message():
    w = nr.weights("N")
    with pytest.raises(NotImplementedError, match=r"only NeighConsensus\(kernel_sizes=\[3,3\], channels=\[16,1\]\) is implemented"):
        ops.NcnWeights(w["conv.0.weight"], w["conv.0.bias"], w["conv.2.weight"], w["conv.2.bias"], "cuda:0")


def _config(ks, ch, sym=1):
    from patch2pix_amd import _lib
    c = _lib.NcnConfig()
    c.n_layers, c.symmetric = len(ks), sym
    for i in range(min(len(ks), 4)):
        c.kernel_size[i], c.channels[i] = ks[i], ch[i]
    return c


def test_create_config_argument_errors():
    """Validation happens before the device is touched: these return their codes on a machine without a GPU."""
    from patch2pix_amd import _lib
    keep = [torch.zeros(16) for _ in range(8)]
    t = _lib.NcnTensors()
    for i in range(4):
        t.w[i], t.b[i] = keep[2 * i].data_ptr(), keep[2 * i + 1].data_ptr()
    out = ctypes.c_void_p()
    good = _config([3, 3], [16, 1])
    assert _lib.p2p_ncn_create_config(None, ctypes.byref(t), ctypes.byref(out)) == -1 and b"null" in _lib.p2p_last_error()
    assert _lib.p2p_ncn_create_config(ctypes.byref(good), None, ctypes.byref(out)) == -1
    assert _lib.p2p_ncn_create_config(ctypes.byref(good), ctypes.byref(t), None) == -1
    for ks, ch in (([7, 3], [16, 1]), ([3, 3], [17, 1]), ([3, 3], [16, 2])):
        c = _config(ks, ch)
        assert _lib.p2p_ncn_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(out)) == -3, (ks, ch)
    c = _config([3, 3, 3, 3], [4, 4, 4, 1])
    c.n_layers = 5
    assert _lib.p2p_ncn_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(out)) == -3
    with pytest.raises(NotImplementedError):
        _lib.check(-3, "p2p_ncn_create_config")
    for ks, ch, n in (([3, 3], [16, 1], 0), ([3, 0], [16, 1], 2), ([3, 3], [-1, 1], 2)):
        c = _config(ks, ch)
        c.n_layers = n
        assert _lib.p2p_ncn_create_config(ctypes.byref(c), ctypes.byref(t), ctypes.byref(out)) == -1, (ks, ch, n)
    empty = _lib.NcnTensors()
    assert _lib.p2p_ncn_create_config(ctypes.byref(good), ctypes.byref(empty), ctypes.byref(out)) == -1
    assert not out.value


def test_queries_return_zero_on_bad_arguments():
    from patch2pix_amd import _lib
    assert _lib.p2p_neigh_consensus_workspace_bytes(None, 4, 4, 4, 4) == 0
    assert _lib.p2p_coarse_workspace_bytes_for(None, 256, 8, 8, 8, 8, 2) == 0
    assert _lib.p2p_ncn_is_generic(None) == -1
    assert _lib.p2p_version() >= 106


@pytest.mark.parametrize("case", list(nr.CASES))
def test_restatement_reproduces_the_reference(case):
    """fp64 against the golden within REF_ERR (that is how REF_ERR is defined), fp32 against fp64 within REF_ERR as well, and
    fp32 against the golden within their sum; the fixture's weights and inputs are the seeded ones."""
    g = nr.load_golden(case)
    sd, lay = nr.weights(case), nr.CASES[case]
    for i in range(len(lay["kernel_sizes"])):
        assert torch.equal(torch.from_numpy(g[f"w{i}"]), sd[f"conv.{2 * i}.weight"])
        assert torch.equal(torch.from_numpy(g[f"b{i}"]), sd[f"conv.{2 * i}.bias"])
    for vol in nr.VOLUMES:
        x, y64 = nr.expected(case, vol)
        assert torch.equal(torch.from_numpy(g[f"x_{vol}"]), x)
        gold = torch.from_numpy(g[f"y_{vol}"]).double()
        y32 = nr.restate(x, sd, lay, torch.float32).double()
        scale = y64.abs().max().item()
        e_gold, e_32, e_both = [(a - b).abs().max().item() for a, b in ((gold, y64), (y32, y64), (y32, gold))]
        print(f"case {case} volume {vol}: golden-f64 {e_gold:.3g}, f32-f64 {e_32:.3g}, f32-golden {e_both:.3g}, scale {scale:.3g}")
        assert e_gold <= nr.REF_ERR[case] * scale and e_32 <= nr.REF_ERR[case] * scale and e_both <= 2 * nr.REF_ERR[case] * scale


def test_symmetric_mode_and_branches_of_the_restatement():
    x, y = nr.expected("N", "thin")
    sd, lay = nr.weights("N"), nr.CASES["N"]
    d, t = nr.restate(x, sd, lay, branch="direct"), nr.restate(x, sd, lay, branch="transposed")
    assert torch.equal(d + t, y) and not torch.equal(d, t)
    assert torch.equal(nr.restate(x, sd, dict(lay, symmetric_mode=False)), d)


def test_holder_spec_of_a_non_released_stack():
    """Patch2Pix builds its `ncn` holder from the layout: config.ncn_config first, else the checkpoint's ncn.conv.* shapes,
    else the released stack -- so such a checkpoint loads with its own keys."""
    from patch2pix_amd.networks import patch2pix as pp
    sd = {"ncn." + k: v for k, v in nr.weights("P").items()}
    lay = pp._ncn_layout_of(Namespace(weights_dict=sd))
    assert lay == nr.CASES["P"]
    holder = pp._Holder(pp._ncn_spec(lay))
    own = holder.state_dict()
    assert {k: tuple(v.shape) for k, v in own.items()} == {k[len("ncn."):]: tuple(v.shape) for k, v in sd.items()}
    holder.load_state_dict({k[len("ncn."):]: v for k, v in sd.items()}, strict=True)
    assert pp._ncn_layout_of(Namespace(weights_dict=sd, ncn_config=dict(nr.CASES["M"]))) == nr.CASES["M"]
    assert pp._ncn_layout_of(Namespace(weights_dict=None)) == ops.RELEASED_NCN_LAYOUT
    assert pp._ncn_layout_of(Namespace(weights_dict={"extract.conv1.weight": torch.zeros(1)})) == ops.RELEASED_NCN_LAYOUT
    assert {k: s for k, (s, _) in pp._NCN_SPEC.items()} == ops.ncn_shapes(ops.RELEASED_NCN_LAYOUT)


def test_synthetic_consensus_weights_are_seeded():
    from patch2pix_amd.utils import synthetic
    a = synthetic.make_ncn_state_dict(5, [5, 3], [7, 1])
    b = synthetic.make_ncn_state_dict(5, [5, 3], [7, 1])
    assert list(a) == ["ncn.conv.0.weight", "ncn.conv.0.bias", "ncn.conv.2.weight", "ncn.conv.2.bias"]
    assert all(torch.equal(a[k], b[k]) for k in a) and tuple(a["ncn.conv.0.weight"].shape) == (5, 7, 1, 5, 5, 5)
