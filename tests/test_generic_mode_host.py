"""Generic regressor mode 'generic_fp16x2' (P2P_REGRESS_GENERIC_FP16X2), host side: the ids and the three dicts, the accept /
refuse matrix of p2p_regressor_set_mode for a generic and a tuned handle (through the emulator's library), chaining two generic
handles in different modes, the workspace query in both modes, a refused allocation on the mode's first selection, the argument
checks of RegressorWeights.set_mode and Patch2Pix.set_fine_mode that need no device, the conditioning of the "range" inputs, and
pack_conv_planes of host_pack.h under AddressSanitizer / UndefinedBehaviorSanitizer in a stand-alone program
(tests/hipemu/generic_pack_test.cpp: its own main, run as a plain process; nothing sanitised is loaded into python).  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import generic_mode_reference as gm
import golden_util as gu
import regressor_reference as rr
from patch2pix_amd import _lib as real
from patch2pix_amd import ops
from patch2pix_amd.networks import patch2pix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, EMU)
import emu_lib  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return emu_lib.load()


def test_ids_and_dicts():
    header = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    ids = {k: int(re.search(rf"#define\s+P2P_REGRESS_{k}\s+(\d+)\b", header).group(1)) for k in ("GENERIC", "GENERIC_FP16X2")}
    assert ids == {"GENERIC": gm.GENERIC, "GENERIC_FP16X2": gm.GENERIC_FP16X2} == {"GENERIC": 16, "GENERIC_FP16X2": 17}
    assert real.REGRESS_MODES_GENERIC == {"generic": 16, "generic_fp16x2": 17} and real.REGRESS_GENERIC == 16
    assert real.REGRESS_MODES == {"f32": 0, "fp16x2": 3, "fp16x2w": 4} and real.REGRESS_MODES_LOSSY == {"fp16": 5}
    assert tuple(sorted({**real.REGRESS_MODES, **real.REGRESS_MODES_LOSSY}.values())) == gm.TUNED_IDS
    assert real.p2p_version() == 112                                                # the ABI version did not move
    assert real.p2p_regressor_set_mode(None, 17) == gm.EINVAL and real.p2p_regressor_get_mode(None) == gm.EINVAL      # NULL: no device needed


def test_set_mode_matrix(emu):
    """Every (handle kind, mode id) pair with the return code of the header; a refused call leaves the mode as it was."""
    gen = gm.emu_handles(emu, "B", mode=gm.GENERIC)[0]
    tuned = emu_lib.regressor_create(emu, rr.sub_params(gu.state_dict(0), "regress_mid."), "fp16x2")
    assert emu.p2p_regressor_get_mode(gen) == 16 and emu.p2p_regressor_get_mode(tuned) == 3
    for mode in (17, 16, 17, 17, 16):
        assert emu.p2p_regressor_set_mode(gen, mode) == gm.OK and emu.p2p_regressor_get_mode(gen) == mode
    assert emu.p2p_regressor_set_mode(gen, 17) == gm.OK
    for mode in gm.TUNED_IDS:
        assert emu.p2p_regressor_set_mode(gen, mode) == gm.EUNSUPPORTED, mode
        assert emu.p2p_regressor_get_mode(gen) == 17
    for mode in (1, 2, 6, 15, 18, -1, 1000):
        assert emu.p2p_regressor_set_mode(gen, mode) == gm.EINVAL, mode
        assert b"unknown mode" in emu.p2p_last_error() and emu.p2p_regressor_get_mode(gen) == 17
    for mode in (16, 17):
        assert emu.p2p_regressor_set_mode(tuned, mode) == gm.EUNSUPPORTED and emu.p2p_regressor_get_mode(tuned) == 3
    assert emu.p2p_regressor_set_mode(tuned, 18) == gm.EINVAL
    assert emu.p2p_regressor_set_mode(tuned, 0) == gm.OK and emu.p2p_regressor_get_mode(tuned) == 0
    gm.destroy(emu, gen, tuned)


def test_first_selection_survives_a_refused_allocation(emu):
    """The planes are packed and uploaded on the first selection: an allocation that fails there is P2P_ENOMEM, the handle stays in
    the exact mode and usable, and the next selection succeeds."""
    try:
        refuse = ctypes.c_int.in_dll(emu, "_ZN6hipemu13refuse_allocsE")
    except ValueError:
        pytest.fail("the emulator library does not export hipemu::refuse_allocs")
    gen = gm.emu_handles(emu, "B", mode=gm.GENERIC)[0]
    p1, p2, props = rr.inputs("emu")
    before = rr.emu_regress(emu, gen, None, p1, p2, props[:3])
    refuse.value = 1
    assert emu.p2p_regressor_set_mode(gen, 17) == gm.ENOMEM and refuse.value == 0
    assert b"hipMalloc" in emu.p2p_last_error() and emu.p2p_regressor_get_mode(gen) == 16
    after = rr.emu_regress(emu, gen, None, p1, p2, props[:3])
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert emu.p2p_regressor_set_mode(gen, 17) == gm.OK and emu.p2p_regressor_get_mode(gen) == 17
    gm.destroy(emu, gen)


def test_chaining_two_modes_is_refused(emu):
    mid, fine = gm.emu_handles(emu, "B", mode=gm.GENERIC)
    assert emu.p2p_regressor_set_mode(fine, 17) == gm.OK
    p1, p2, props = rr.inputs("emu")
    with pytest.raises(AssertionError, match="returned -1"):
        rr.emu_regress(emu, mid, fine, p1, p2, props[:3])
    msg = emu.p2p_last_error().decode()
    assert "different arithmetic modes" in msg and "16" in msg and "17" in msg, msg
    assert emu.p2p_regressor_set_mode(mid, 17) == gm.OK
    out = rr.emu_regress(emu, mid, fine, p1, p2, props[:3])
    assert bool(torch.isfinite(out["raw2"]).all())
    gm.destroy(emu, mid, fine)


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_workspace_query_follows_the_mode(case, emu):
    """Per proposal the new mode adds spp x (n_conv - 1) words; the unit of 8, the cap of 256 and P2P_ENOMEM below one unit stay."""
    c = rr.CASES[case]
    extra = 4 * (2 if c["feat_comb"] == "post" else 1) * (len(c["conv_dims"]) - 1)
    mid = gm.emu_handles(emu, case, mode=gm.GENERIC)[0]
    q = lambda n: emu.p2p_regress_workspace_bytes_for(mid, n)
    exact = {n: q(n) for n in (1, 8, 9, 61, 256, 100000)}
    assert exact[1] == exact[8] and exact[9] == 2 * exact[8] and exact[61] == 8 * exact[8] and exact[100000] == exact[256] == 32 * exact[8]
    assert emu.p2p_regressor_set_mode(mid, 17) == gm.OK
    for n, b in exact.items():
        assert q(n) == b + extra * ((min(n, 256) + 7) // 8 * 8), (n, q(n), b)
    assert q(0) == 0
    if extra:
        p1, p2, props = rr.inputs("emu")
        with pytest.raises(AssertionError, match="returned -4"):          # the exact mode's unit is below the new mode's
            rr.emu_regress(emu, mid, None, p1, p2, props[:3], ws_bytes=exact[8])
    assert emu.p2p_regressor_set_mode(mid, 16) == gm.OK
    assert {n: q(n) for n in exact} == exact
    gm.destroy(emu, mid)


def _weights(generic):
    w = ops.RegressorWeights.__new__(ops.RegressorWeights)
    w.handle, w.generic, w.device = None, generic, torch.device("cpu")
    return w


def test_regressor_weights_set_mode_argument_checks():
    """Names of the other kind: NotImplementedError; unknown names: ValueError -- both before the library is asked (the handle is None)."""
    gen, tuned = _weights(True), _weights(False)
    for name in ("f32", "fp16x2", "fp16x2w", "fp16"):
        with pytest.raises(NotImplementedError):
            gen.set_mode(name)
    for name in ("generic", "generic_fp16x2"):
        with pytest.raises(NotImplementedError):
            tuned.set_mode(name)
    for w in (gen, tuned):
        for name in ("generic_fp16", "GENERIC", "", "bf16x2", None):
            with pytest.raises(ValueError):
                w.set_mode(name)


def _model(layout, regressors=True):
    m = object.__new__(patch2pix.Patch2Pix)
    d = m.__dict__
    d["_packed"], d["regress_mid"] = None, (object() if regressors else None)
    if regressors:
        d["_layout"] = layout
    return m


def test_set_fine_mode_argument_checks(monkeypatch):
    monkeypatch.delenv("P2P_REGRESS_GENERIC_MODE", raising=False)
    monkeypatch.delenv("P2P_REGRESS_MODE", raising=False)
    assert callable(patch2pix.Patch2Pix.set_fine_mode) and isinstance(patch2pix.Patch2Pix.fine_mode, property)
    ck = rr.checkpoint("A")
    generic = _model(ops.regressor_layout(ck["regressor_config"], ck["feat_idx"]))
    released = _model(ops.RELEASED_LAYOUT)
    assert generic._layout != ops.RELEASED_LAYOUT
    assert generic.fine_mode == "generic" and released.fine_mode == "fp16x2w"
    for m, good, other in ((generic, ("generic_fp16x2", "generic"), ("f32", "fp16x2", "fp16x2w", "fp16")),
                           (released, ("f32", "fp16", "fp16x2w"), ("generic", "generic_fp16x2"))):
        for name in ("nope", "", None, 17):
            with pytest.raises(ValueError):
                m.set_fine_mode(name)
        for name in other:
            with pytest.raises(NotImplementedError):
                m.set_fine_mode(name)
        assert "_fine_mode" not in m.__dict__                      # nothing changed so far
        for name in good:                                          # nothing is packed: the choice is recorded for the next pack
            m.set_fine_mode(name)
            assert m.fine_mode == name
    none = _model(None, regressors=False)
    with pytest.raises(ValueError, match="no regressors"):
        none.set_fine_mode("generic")
    assert none.fine_mode is None
    monkeypatch.setenv("P2P_REGRESS_GENERIC_MODE", "generic_fp16x2")
    assert _model(generic._layout).fine_mode == "generic_fp16x2" and _model(ops.RELEASED_LAYOUT).fine_mode == "fp16x2w"


@pytest.mark.parametrize("variant", gm.VARIANTS)
def test_range_variants_are_well_conditioned(variant):
    """A condition on the inputs the range tests add (case A with layer 0's BatchNorm changed): the fp32 restatement within
    1e-4 px / 1e-6 of its own fp64 evaluation on the pyramids and proposals of the emulated and the GPU tests, mid level and the
    fine level from the fp64 mid matches (tests/test_regressor_configs_host.py does the same for the unmodified checkpoints)."""
    case = "A"
    p32, p64 = gm.variant_params(case, variant), gm.variant_params(case, variant, torch.float64)
    for name in ("emu", "gpu"):
        p1, p2, props = rr.inputs(name)
        r64 = gm.levels_of(p64, p1, p2, props, case)
        r32 = gm.levels_of(p32, p1, p2, props, case, mid_out=r64[0].float())
        cond = [(a.double() - b).abs().max().item() for a, b in zip(r32, r64)]
        print(f"case {case} variant {variant} {name}: coord {max(cond[0], cond[2]):.3g} px score {max(cond[1], cond[3]):.3g}")
        assert max(cond[0], cond[2]) <= rr.COND_COORD and max(cond[1], cond[3]) <= rr.COND_SCORE, cond
        # the variant does what it is for: layer 0's stored magnitudes moved by the factor (uniform), or one channel leads (outlier)
        assert torch.isfinite(r32[2]).all() and torch.isfinite(r32[3]).all()


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    cxx = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    exe = str(tmp_path_factory.mktemp("generic_pack") / "generic_pack_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", EMU, os.path.join(EMU, "generic_pack_test.cpp"),
           os.path.join(EMU, "hipemu.cpp"), "-pthread", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode and "libclang_rt." in res.stdout:      # the link step cannot find the sanitizer runtime: no unsanitized build instead
        pytest.skip("the sanitizer runtime is missing: " + res.stdout.strip()[-400:])
    assert res.returncode == 0, res.stdout
    return exe


def test_pack_conv_planes_runs_clean_under_the_sanitizers(pack_program):
    res = subprocess.run([pack_program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "generic_pack_test: ok" in res.stdout, res.stdout
    assert "runtime error" not in res.stdout and "ERROR: " not in res.stdout, res.stdout
