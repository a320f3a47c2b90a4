"""The GEMM operand buffers of the fine and the coarse stage, decoded, on the MI355X:  pytest -m gpu

The checks of tests/test_stage_buffers_emulated.py (see there; the decoders, references and assertions are in
tests/stage_reference.py) at the GPU's shapes -- a 64 x 96 pair, launches of 1, 7, 9 and 41 proposals, three device-count
tables -- plus the launch of more than one chunk, which only the GPU can afford.  Every call gets a workspace of exactly
the size the library asks for, filled with 0xFF, and a 4 KiB guard band behind it."""
import pytest
import torch

import golden_util as gu
import stage_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X (run on the GPU box)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from patch2pix_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def sd():
    return gu.state_dict(0)


@pytest.fixture(scope="module")
def weights(dev, sd):
    from patch2pix_amd import ops
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    out = {}
    for mode in ("fp16x2w", "fp16x2"):
        out[mode] = (ops.RegressorWeights(sub("regress_mid."), dev), ops.RegressorWeights(sub("regress_fine."), dev))
        for w in out[mode]:
            w.set_mode(mode)
    return out


@pytest.fixture(scope="module")
def handles(weights):
    return {m: (a.handle, b.handle) for m, (a, b) in weights.items()}


@pytest.fixture(scope="module")
def ncn_weights(dev, sd):
    from patch2pix_amd import ops
    return ops.NcnWeights(*[sd[f"ncn.conv.{k}"] for k in ("0.weight", "0.bias", "2.weight", "2.bias")], dev)


@pytest.fixture(scope="module")
def ncn(ncn_weights):
    return ncn_weights.handle


@pytest.fixture(scope="module")
def launches(lib, dev, handles):
    return sr.FineLaunches("gpu", lib, dev, handles)


def test_restated_workspace_sizes(lib, ncn):
    from patch2pix_amd import _lib
    sr.check_workspace_formulas(lib, ncn, _lib.REGRESS_MODES)


@pytest.mark.parametrize("two", [False, True], ids=["one_level", "two_levels"])
@pytest.mark.parametrize("n", sr.CONFIG["gpu"]["ns"])
def test_host_counts(n, two, launches):
    sr.check_host_counts(launches, n, two)


@pytest.mark.parametrize("i", sr.CONFIG["gpu"]["singles"])
def test_launch_independence(i, launches):
    sr.check_independence(launches, i)


def test_prefix_launch_has_the_same_bits(launches):
    for i in range(9):
        sr.check_independence(launches, i, 0, 9)


@pytest.mark.parametrize("stride,counts", [(3, [2, -1, 1]), (11, [11, 0, 5, 3]), (8, [0, 0, 8, 1])])
def test_device_counts(stride, counts, lib, dev, handles):
    sr.check_device_counts(lib, dev, *handles["fp16x2w"], stride=stride, counts=counts)


def test_more_than_one_chunk(lib, dev, handles):
    """n = 3403 on one 48 x 64 pair, two levels: chunks of 1792 and 1611 proposals share U, the second with 202 row blocks
    (another position stride than the first one's 224) and a partly filled last block.  Decoded with the LAST chunk's
    row-block count, on the device.  No emulated twin: 6806 proposal-levels at 3-10 CPU-seconds each."""
    from patch2pix_amd.utils import synthetic
    n, H, W = 3403, 48, 64
    assert sr.wino_chunks(n) == [(0, 1792), (1792, 3403)]
    p0, p1 = sr.wino_chunks(n)[-1]
    mblocks = (p1 - p0 + 7) // 8
    assert mblocks == 202 and (p1 - p0) % 8 == 3
    mid, fine = handles["fp16x2w"]
    pyr1, pyr2 = synthetic.make_pyramid(81, H, W)[:4], synthetic.make_pyramid(82, H, W)[:4]
    props = sr.proposals(H, W, n, seed=8)
    res = sr.run_fine(lib, mid, fine, pyr1, pyr2, props, dev)
    assert sr.guard_intact(res), "the guard band behind the workspace was written"
    tail = list(range(p1 - p0, 8 * mblocks))
    assert len(tail) == 5
    hi, lo, hinv = sr.decode_U(res["ws"], n, mblocks, tail)
    assert sr.is_zero_bits(hi) and sr.is_zero_bits(lo) and sr.is_zero_bits(hinv), "the five rows no proposal owns"
    v1, v2 = sr.decode_V(res["ws"], n, 0), sr.decode_V(res["ws"], n, 1)
    assert bool(torch.isfinite(v1).all()) and bool(torch.isfinite(v2).all())
    assert not bool((res["matches2"] == sr.MARK).any())

    def single(i, level2):       # proposal i alone: the mid regressor on its proposal, or the fine one on its mid match
        if level2:
            return sr.run_fine(lib, fine, None, pyr1, pyr2, res["matches1"][i:i + 1].clone(), dev)
        return sr.run_fine(lib, mid, None, pyr1, pyr2, props[i:i + 1], dev)

    last = [1792, 3000, 3402]
    hi, lo, hinv = sr.decode_U(res["ws"], n, mblocks, [i - p0 for i in last])
    sr.assert_planes_sane(hi, lo, 2.0 ** 13, "rows of the last chunk")
    sr.assert_pow2(hinv, "last chunk")
    for k, i in enumerate(last):
        one = single(i, True)
        shi, slo, shinv = sr.decode_U(one["ws"], 1, 1, [0])
        rows = slice(16 * k, 16 * (k + 1))
        assert torch.equal(hi[rows].view(torch.int16), shi.view(torch.int16)) and torch.equal(lo[rows].view(torch.int16), slo.view(torch.int16)), \
            f"proposal {i}: U rows differ from its single launch"
        assert torch.equal(hinv[k:k + 1], shinv), f"proposal {i}: hinv"
        assert torch.equal(v2[i], sr.decode_V(one["ws"], 1, 0)[0]), f"proposal {i}: V of level 2"
        assert torch.equal(res["matches2"][i], one["matches1"][0]) and torch.equal(res["probs2"][i], one["probs1"][0])
    for i in (0, 1791) + tuple(last):
        assert torch.equal(v1[i], sr.decode_V(single(i, False)["ws"], 1, 0)[0]), f"proposal {i}: V of level 1"
    for i in (0, 1791):
        assert torch.equal(v2[i], sr.decode_V(single(i, True)["ws"], 1, 0)[0]), f"proposal {i} (first chunk): V of level 2"


@pytest.mark.parametrize("mode", ["fp16x2w", "fp16x2"])
def test_fine_values_against_fp64(mode, launches, sd):
    sr.assert_fine_values(launches, mode, sd)


@pytest.mark.parametrize("mode", ["fp16x2w", "fp16x2"])
def test_emulator_inputs_on_the_gpu(mode, lib, dev, handles, sd):
    """The inputs of tests/test_stage_buffers_emulated.py themselves (16 x 24, its nine proposals) on the MI355X, held to the
    bars of those inputs: next to that file's "stage[emu]" lines the "stage[emu inputs on the MI355X]" lines are the
    same-input comparison of the stand-in's arithmetic with the hardware's ("Numeric domain of the fp16x2 paths")."""
    sr.assert_fine_values(sr.FineLaunches("emu", lib, dev, handles), mode, sd, label="emu inputs on the MI355X")


@pytest.mark.parametrize("case", sr.COARSE_CASES, ids=lambda c: f"k{c[5]}")
def test_coarse_planes(case, lib, dev, ncn):
    sr.check_coarse_case(lib, dev, ncn, case, "gpu")


def test_coarse_planes_are_scale_free(lib, dev, ncn):
    sr.check_coarse_scale_free(lib, dev, ncn, sr.COARSE_CASES[1])


def test_coarse_zero_column_gives_zero_planes(lib, dev, ncn):
    sr.check_coarse_zero_column(lib, dev, ncn, sr.COARSE_CASES[2])
