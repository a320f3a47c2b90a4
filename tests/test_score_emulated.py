"""The pair score (score_cells_kernel / score_pair_kernel of csrc/score.hip behind p2p_coarse_score_batch) executed on the CPU
by the test-suite's HIP stand-in (tests/hipemu) on cases S, W, N and D of tests/score_reference.py with all three
normalisations: raw cell scores bit-equal to torch.max, softmax cell scores bit-equal to the scores of the emulated
p2p_coarse_matches_batch, l1 cells and every pair score within the bars of the fp64 yardstick and of the unmodified
reference's scalars (tests/golden/score_*.npz), a pair alone equal to the pair in its batch, cell_scores = NULL."""
import os
import sys

import pytest

import score_reference as sr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402

CASE_NORMS = [(c, n) for c in sr.HOST_CASES for n in sr.NORMS]
IDS = [f"{c}-{sr.norm_tag(n)}" for c, n in CASE_NORMS]


@pytest.fixture(scope="module")
def emu():
    return sr.bind(emu_lib.load())


@pytest.mark.parametrize("case,normalize", CASE_NORMS, ids=IDS)
def test_scores(case, normalize, emu):
    sr.check_case(emu, case, normalize)


@pytest.mark.parametrize("case,normalize", CASE_NORMS, ids=IDS)
def test_scores_against_reference_golden(case, normalize, emu):
    sr.check_against_golden(emu, case, normalize)
