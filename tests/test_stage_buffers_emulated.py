"""The GEMM operand buffers of the fine and the coarse stage, decoded: the kernels' own code on the CPU (tests/hipemu).

Every other test of the two-plane paths is end to end.  Here the caller's workspace is filled with 0xFF (plus a 4 KiB
guard band behind it), a call is made through the C ABI, and the buffers one kernel leaves for the next are read back and
decoded by tests/stage_reference.py, which restates the layouts from the header comments: the Winograd-transformed conv2
input U with its inverse scales hinv and the pooled features V of the fine stage, the normalised feature planes of the
coarse stage.  Exact checks (zero-filled tail and pad rows, canonical two-plane splits, bounds, launch independence bit
for bit, untouched guard bands) and value checks against fp64 whose bars are a measured multiple of the fp32
restatement's own error (stage_reference.R_MEASURED; DESIGN.md, "Numeric domain of the fp16x2 paths").

tests/test_gpu_stage_buffers.py runs the same checks on the MI355X at larger shapes and adds the multi-chunk launch
(n = 3403): at 3-10 CPU-seconds per proposal and level that one is out of the emulator's reach and has no twin here.
This file stays within about 60 proposal-levels: a 16 x 24 pair, launches of 1 and 9 proposals.

Mutations of the kernels, each run on a scratch copy of csrc/ (nothing of them committed), and the tests they turn red:
(a) wino_zero_tail_kernel not launched             -> test_host_counts (all four cases), test_device_counts
(b) the a0 b1 MFMA dropped from WSLAB_             -> test_fine_values_against_fp64[fp16x2w]: e_V 2.1e-4 against a bar of 1.8e-6
(c) one sign of the A^T coefficients flipped       -> test_fine_values_against_fp64[fp16x2w]: e_V 1.0
(d) the XOR swizzle removed from wino_zero_tail_kernel's inblk only -> nothing, and nothing can: a row's four lanes
    (lane & 3 = 0..3) write its four 16-byte slots whether or not the index is XORed with a constant of the row, and all of
    them write zeros -- the same bytes get the same values, the mutant is the same program.  The address mutation that does
    change bytes, (d') the row base of the zero-fill moved by one proposal (j -> j - 1), turns test_host_counts (all four)
    and test_device_counts red.
(e) the pad fill of prep_kernel skipped            -> test_coarse_planes (all three cases)"""
import os
import sys

import pytest

import golden_util as gu
import stage_reference as sr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402
from patch2pix_amd import _lib as real  # noqa: E402

DEV = "cpu"


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


@pytest.fixture(scope="module")
def sd():
    return gu.state_dict(0)


@pytest.fixture(scope="module")
def handles(emu, sd):
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    return {m: (emu_lib.regressor_create(emu, sub("regress_mid."), m), emu_lib.regressor_create(emu, sub("regress_fine."), m))
            for m in ("fp16x2w", "fp16x2")}


@pytest.fixture(scope="module")
def ncn(emu, sd):
    return emu_lib.ncn_create(emu, sd)


@pytest.fixture(scope="module")
def launches(emu, handles):
    return sr.FineLaunches("emu", emu, DEV, handles)


def test_restated_workspace_sizes(emu, ncn):
    sr.check_workspace_formulas(emu, ncn, real.REGRESS_MODES)


@pytest.mark.parametrize("two", [False, True], ids=["one_level", "two_levels"])
@pytest.mark.parametrize("n", sr.CONFIG["emu"]["ns"])
def test_host_counts(n, two, launches):
    sr.check_host_counts(launches, n, two)


@pytest.mark.parametrize("i", sr.CONFIG["emu"]["singles"])
def test_launch_independence(i, launches):
    sr.check_independence(launches, i)


def test_device_counts(emu, handles):
    sr.check_device_counts(emu, DEV, *handles["fp16x2w"], stride=3, counts=[2, -1, 1])


@pytest.mark.parametrize("mode", ["fp16x2w", "fp16x2"])
def test_fine_values_against_fp64(mode, launches, sd):
    sr.assert_fine_values(launches, mode, sd)


@pytest.mark.parametrize("case", sr.COARSE_CASES, ids=lambda c: f"k{c[5]}")
def test_coarse_planes(case, emu, ncn):
    sr.check_coarse_case(emu, DEV, ncn, case, "emu")


def test_coarse_planes_are_scale_free(emu, ncn):
    sr.check_coarse_scale_free(emu, DEV, ncn, sr.COARSE_CASES[1])


def test_coarse_zero_column_gives_zero_planes(emu, ncn):
    sr.check_coarse_zero_column(emu, DEV, ncn, sr.COARSE_CASES[2])
