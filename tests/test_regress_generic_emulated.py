"""The generic regressor kernels (csrc/regress_generic.hip) compiled for the host and run on the CPU (tests/hipemu): cases A-D
of tests/regressor_reference.py against the fp32 restatement at the project's bars, the released configuration forced through
the generic path on the reference's forward_fine_match golden, and chunk-size invariance.  Case E runs on the GPU only."""
import os
import sys

import pytest
import torch

import golden_util as gu
import regressor_reference as rr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import emu_lib  # noqa: E402

# 48x64 pyramids; three proposals, the second one's windows across the top-left / bottom-right image corners (+ 8 for chunking)
PROPS = rr.inputs("emu")[2][:3]


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


@pytest.fixture(scope="module")
def pyramids():
    return rr.inputs("emu")[:2]


def _handles(emu, case):
    sd = rr.checkpoint(case)["state_dict"]
    out = []
    for prefix in ("regress_mid.", "regress_fine."):
        st, h = rr.create_config(emu, rr.sub_params(sd, prefix), rr.CASES[case])
        assert st == 0, emu.p2p_last_error()
        out.append(h)
    return out


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_generic_cases_against_restatement(case, emu, pyramids):
    mid, fine = _handles(emu, case)
    assert emu.p2p_regressor_get_mode(mid) == 16
    out = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], PROPS)
    rr.check_levels(out, pyramids[0], pyramids[1], PROPS, case, "emulated")
    for h in (mid, fine):
        emu.p2p_regressor_destroy(h)


def test_released_configuration_on_reference_golden(emu):
    """Case R: the released shapes through p2p_regressor_create_config, on the golden test_kernels_emulated.py uses for the
    tuned kernels -- integer proposals through the mid regressor, float proposals through the fine one."""
    sd = gu.state_dict(0)
    g = gu.load("fine_48x64")
    p1, p2 = gu.fine_inputs(g)
    n = 3
    for tag, prefix in (("int_mid", "regress_mid."), ("float_fine", "regress_fine.")):
        st, reg = rr.create_config(emu, rr.sub_params(sd, prefix), rr.CASES["R"])
        assert st == 0, emu.p2p_last_error()
        props = torch.from_numpy(g[tag + "_in"][:n])
        out = rr.emu_regress(emu, reg, None, p1, p2, props)
        dc = (out["matches1"] - torch.from_numpy(g[tag + "_matches"][:n])).abs().max().item()
        ds = (out["probs1"] - torch.from_numpy(g[tag + "_probs"][:n])).abs().max().item()
        print(f"case R {tag}: coord {dc:.3g} px score {ds:.3g}")
        assert dc <= rr.COORD_TOL and ds <= rr.SCORE_TOL
        emu.p2p_regressor_destroy(reg)


@pytest.mark.parametrize("case", ["A", "C"])
def test_chunk_size_does_not_change_a_bit(case, emu, pyramids):
    """3 + 8 proposals with the smallest workspace the library accepts (chunks of 8) and with the full one."""
    mid, fine = _handles(emu, case)
    props = rr.inputs("emu")[2]
    unit, full = emu.p2p_regress_workspace_bytes_for(mid, 8), emu.p2p_regress_workspace_bytes_for(mid, 11)
    assert full == 2 * unit
    a = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], props, ws_bytes=unit)
    b = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], props, ws_bytes=full)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    alone = rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], props[4:5])
    assert torch.equal(alone["raw1"][0], a["raw1"][4]) and torch.equal(alone["raw2"][0], a["raw2"][4])
    # below one unit: P2P_ENOMEM
    with pytest.raises(AssertionError, match="returned -4"):
        rr.emu_regress(emu, mid, fine, pyramids[0], pyramids[1], props, ws_bytes=unit - 128)
    for h in (mid, fine):
        emu.p2p_regressor_destroy(h)
