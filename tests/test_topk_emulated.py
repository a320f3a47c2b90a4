"""The top-k match extraction (match_cols_topk_kernel / match_rows_topk_kernel of csrc/matches.hip behind
p2p_coarse_matches_topk_batch) executed on the CPU by the test-suite's HIP stand-in (tests/hipemu): the torch restatement
on every case of tests/topk_reference.py (of the one-candidate entry as well), the unmodified reference's outputs (tests/golden/topk_*.npz), the identity of
topk = 1 with the one-candidate kernels, and the argument checks."""
import os
import sys

import pytest
import torch

import topk_reference as tr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return tr.bind(emu_lib.load())


@pytest.mark.parametrize("case", list(tr.CASES))
def test_topk_against_restatement(case, emu):
    tr.check_against_restatement(emu, case)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_one_candidate_against_restatement(case, emu):
    tr.check_one_candidate_against_restatement(emu, case)


@pytest.mark.parametrize("case", tr.GOLDEN_CASES)
def test_topk_against_reference_golden(case, emu):
    tr.check_against_golden(emu, case)


@pytest.mark.parametrize("case", list(tr.CASES))
def test_topk_1_is_the_one_candidate_kernels(case, emu):
    tr.check_top1_identity(emu, case)


def test_topk_argument_errors(emu):
    """topk outside 1..8 or beyond min(nA, nB), and the checks of the one-candidate entry: P2P_EINVAL (-1) with a message."""
    corr = torch.zeros(2, 2, 3, 3, 4)
    delta = torch.zeros(2, 2, 3, 3, 4, dtype=torch.uint8)
    m = torch.zeros(2, 8 * 18, 4, dtype=torch.int64)
    s = torch.zeros(2, 8 * 18)
    p = emu_lib.ptr

    def call(topk, corr_=corr, delta_=delta, batch=2, dims=(2, 3, 3, 4), ksize=2, m_=m, s_=s):
        return emu.p2p_coarse_matches_topk_batch(p(corr_), p(delta_), batch, *dims, ksize, 8, 1, topk, 1, p(m_), p(s_), None)

    for topk in (0, -1, 9, 64):
        assert call(topk) == -1, topk
        assert b"topk" in emu.p2p_last_error() and b"1 to 8" in emu.p2p_last_error()
    assert call(7) == -1 and b"exceeds the 6 cells" in emu.p2p_last_error()          # nA = 6 < 7 <= 8
    assert call(3, dims=(6, 1, 1, 2)) == -1 and b"exceeds the 2 cells" in emu.p2p_last_error()
    assert call(2, delta_=None) == -1 and b"delta required" in emu.p2p_last_error()
    assert call(2, corr_=None) == -1 and b"null" in emu.p2p_last_error()
    assert call(2, m_=None) == -1 and call(2, s_=None) == -1
    assert call(2, batch=0) == -1 and b"batch" in emu.p2p_last_error()
    assert call(2, dims=(2, 0, 3, 4)) == -1 and b"bad sizes" in emu.p2p_last_error()
    assert call(6) == 0, emu.p2p_last_error()                                        # topk = min(nA, nB) is allowed
    assert call(2, delta_=None, ksize=1) == 0, emu.p2p_last_error()
