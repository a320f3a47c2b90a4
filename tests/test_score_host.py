"""The pair score (p2p_coarse_score_batch, Patch2Pix.cal_coarse_score) without a GPU: the test infrastructure against the
unmodified reference's fixtures (tests/golden/score_*.npz), the condition on the signed l1 inputs, and the argument checks of
the Python layer and of the real library, none of which touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import score_reference as sr

CASE_NORMS = [(c, n) for c in sr.HOST_CASES for n in sr.NORMS]
IDS = [f"{c}-{sr.norm_tag(n)}" for c, n in CASE_NORMS]


@pytest.fixture(scope="module")
def real_lib():
    """The real library, built if need be (importing the package needs it); nothing here launches a kernel."""
    from patch2pix_amd import build
    build.build(verbose=False)
    from patch2pix_amd import _lib
    return _lib


@pytest.mark.parametrize("case,normalize", CASE_NORMS, ids=IDS)
def test_restatement_equals_the_reference(case, normalize):
    """The fixture's inputs are the generator's; the restatement in fp32 (the reference's own arithmetic) gives the
    reference's scalar within the bar, and so does the fp64 yardstick: the reference's own fp32 error is inside the bars that
    the library is held to, cell by cell and pair by pair."""
    g = np.load(sr.golden_name(case))
    corr = sr.inputs(case, normalize)
    assert np.array_equal(g[f"corr_{sr.kind_of(case, normalize)}"], corr.numpy()), "the generator no longer gives the fixture's inputs"
    ref = float(g[f"score_{sr.norm_tag(normalize)}"])
    cells32, pair32, scalar32 = sr.restate(corr, normalize, torch.float32)
    cells64, pair64, scalar64 = sr.restate(corr, normalize)
    assert cells32.dtype == torch.float32 and cells32.shape == (corr.shape[0], corr.shape[1] * corr.shape[2] + corr.shape[3] * corr.shape[4])
    sr.assert_within("fp32 restatement against the reference", scalar32, ref, case, normalize)
    sr.assert_within("reference against the fp64 yardstick", ref, scalar64, case, normalize)
    sr.assert_within("fp32 cells against the fp64 yardstick", cells32, cells64, case, normalize)
    sr.assert_within("fp32 pairs against the fp64 yardstick", pair32, pair64, case, normalize)
    sr.assert_within("mean of the pair scores against the scalar", pair64.mean(), scalar64, case, normalize)
    if sr.is_unit_range(case, normalize):
        assert 0.0 <= float(cells64.min()) and float(cells64.max()) <= 1.0 + 1e-12


def test_l1_inputs_are_well_conditioned():
    """Every row and column of the signed l1 volume has |sum x + 1e-4| >= 0.1 sum |x| (and the volume is signed, with a
    negative row and column sum); the other l1 volumes are non-negative."""
    corr = sr.inputs("D", "l1")
    assert sr.kind_of("D", "l1") == "signed" and sr.l1_condition(corr) >= sr.L1_CONDITION
    X = corr.reshape(corr.shape[0], 35, 54)
    p = sr.PLANTED
    assert bool((X < 0).any()) and bool((X.sum(dim=2)[:, p["neg_row"]] < 0).all()) and bool((X.sum(dim=1)[:, p["neg_col"]] < 0).all())
    assert bool((X[:, p["zero_row"]] == 0).all()) and bool((X[:, :, p["zero_col"]] == 0).all())
    # the l1 score of such a slice is min(x) / d, that of a zero slice 0
    cells, _, _ = sr.restate(corr, "l1")
    assert bool((cells[:, p["neg_row"]] > 0).all()) and bool((cells[:, 35 + p["neg_col"]] > 0).all())
    assert bool((cells[:, p["zero_row"]] == 0).all()) and bool((cells[:, 35 + p["zero_col"]] == 0).all())
    for case in ("S", "W", "N", "T"):
        assert bool((sr.inputs(case, "l1") >= 0).all())


def test_unknown_normalize_is_a_value_error(real_lib):
    """Checked before anything else looks at the tensor: CPU tensors, no device."""
    from patch2pix_amd import ops
    from patch2pix_amd.networks.patch2pix import Patch2Pix
    corr = torch.zeros(1, 2, 2, 2, 2)
    for bad in ("l2", "Softmax", "", 1, ["softmax"]):
        with pytest.raises(ValueError, match="normalize"):
            ops.coarse_score_batch(corr, bad)
        with pytest.raises(ValueError, match="normalize"):
            Patch2Pix.cal_coarse_score(None, corr.unsqueeze(1), normalize=bad)
        with pytest.raises(ValueError, match="normalize"):
            ops.score_norm(bad)
    assert [ops.score_norm(n) for n in sr.NORMS] == [sr.NORM_CODE[n] for n in sr.NORMS] == [0, 1, 2]


def test_entry_point_argument_errors(real_lib):
    """P2P_EINVAL (-1) for null pointers, sizes <= 0 and an unknown normalisation, P2P_ENOMEM (-4) for a missing or short
    workspace when cell_scores is NULL -- all before the device is touched (placeholder addresses, no GPU here)."""
    _lib = real_lib
    lib = sr.bind(_lib.lib)
    p = ctypes.c_void_p(256)          # never dereferenced on the host

    def call(corr=p, batch=2, dims=(2, 3, 3, 4), norm=1, cells=p, pair=p, ws=None, ws_bytes=0):
        return lib.p2p_coarse_score_batch(corr, batch, *dims, norm, cells, pair, ws, ws_bytes, None)

    assert call(corr=None) == -1 and b"null" in lib.p2p_last_error()
    assert call(pair=None) == -1 and b"null" in lib.p2p_last_error()
    for batch in (0, -1, 65536):
        assert call(batch=batch) == -1 and b"batch" in lib.p2p_last_error()
    for dims in ((0, 3, 3, 4), (2, -1, 3, 4), (2, 3, 0, 4), (2, 3, 3, 0)):
        assert call(dims=dims) == -1 and b"bad sizes" in lib.p2p_last_error()
    for norm in (-1, 3, 16):
        assert call(norm=norm) == -1 and b"normalisation" in lib.p2p_last_error()
    need = lib.p2p_coarse_score_workspace_bytes(2, 2, 3, 3, 4)
    assert need == 2 * (6 + 12) * 4
    assert call(cells=None) == -4 and b"workspace" in lib.p2p_last_error()
    assert call(cells=None, ws=p, ws_bytes=need - 1) == -4
    assert call(cells=None, ws=ctypes.c_void_p(258), ws_bytes=need) == -1 and b"aligned" in lib.p2p_last_error()
    for bad in ((0, 2, 3, 3, 4), (65536, 2, 3, 3, 4), (2, 0, 3, 3, 4), (2, 2, 3, 3, -4)):
        assert lib.p2p_coarse_score_workspace_bytes(*bad) == 0
    assert _lib.SCORE_NORMS == sr.NORM_CODE
