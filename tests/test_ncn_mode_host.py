"""Generic consensus mode 'generic_fp16x2' (P2P_COARSE_GENERIC_FP16X2), host side: the id and the name tables, the environment
variable, every error path of NcnWeights.set_mode and Patch2Pix.set_coarse_mode on handle-less objects, the conditioning of the
inputs tests/ncn_mode_reference.py adds, and pack_conv4d_planes of csrc/host_pack.h against its definition (a stand-alone
program, tests/ncn_pack_dump.cpp).  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ncn_mode_reference as nm
import ncn_reference as nr
from patch2pix_amd import _lib as real
from patch2pix_amd import ops
from patch2pix_amd.networks import patch2pix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ids_and_name_tables():
    header = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert int(re.search(r"#define\s+P2P_COARSE_GENERIC_FP16X2\s+(\d+)\b", header).group(1)) == nm.GENERIC_FP16X2 == 17
    assert real.COARSE_MODES == {"fp16x2": 0, "fp16": 1} and real.COARSE_MODES_GENERIC == {"generic": 0, "generic_fp16x2": 17}
    assert real.p2p_version() == 112
    assert real.p2p_ncn_set_mode(None, 17) == nm.EINVAL and real.p2p_ncn_get_mode(None) == -1      # NULL: no device needed
    assert ops.coarse_mode_id("fp16x2") == 0 and ops.coarse_mode_id("fp16") == 1
    for name in ("generic", "generic_fp16x2"):                 # coarse_mode_id keeps to the tuned names
        with pytest.raises(ValueError):
            ops.coarse_mode_id(name)


def test_environment_variable(monkeypatch):
    monkeypatch.delenv("P2P_COARSE_GENERIC_MODE", raising=False)
    monkeypatch.setenv("P2P_COARSE_MODE", "fp16")
    assert ops.default_coarse_generic_mode() == "generic" and ops.default_coarse_mode() == "fp16"
    monkeypatch.setenv("P2P_COARSE_GENERIC_MODE", "generic_fp16x2")
    monkeypatch.delenv("P2P_COARSE_MODE", raising=False)
    assert ops.default_coarse_generic_mode() == "generic_fp16x2" and ops.default_coarse_mode() == "fp16x2"
    assert _model(nr.CASES["N"]).coarse_mode == "generic_fp16x2" and _model(ops.RELEASED_NCN_LAYOUT).coarse_mode == "fp16x2"


def _weights(generic):
    w = ops.NcnWeights.__new__(ops.NcnWeights)
    w.handle, w.generic, w.device = None, generic, torch.device("cpu")
    return w


def test_ncn_weights_set_mode_argument_checks():
    gen, tuned = _weights(True), _weights(False)
    for name in ("fp16x2", "fp16"):
        with pytest.raises(NotImplementedError):
            gen.set_mode(name)
    for name in ("generic", "generic_fp16x2"):
        with pytest.raises(NotImplementedError):
            tuned.set_mode(name)
    for w in (gen, tuned):
        for name in ("half", "GENERIC", "generic_fp16", "", None, 17):
            with pytest.raises(ValueError):
                w.set_mode(name)


def _model(layout):
    m = object.__new__(patch2pix.Patch2Pix)
    m.__dict__["_packed"], m.__dict__["_ncn_layout"] = None, layout
    return m


def test_set_coarse_mode_argument_checks(monkeypatch):
    monkeypatch.delenv("P2P_COARSE_GENERIC_MODE", raising=False)
    monkeypatch.delenv("P2P_COARSE_MODE", raising=False)
    generic, released = _model(nr.CASES["P"]), _model(ops.RELEASED_NCN_LAYOUT)
    assert generic._ncn_layout != ops.RELEASED_NCN_LAYOUT
    assert generic.coarse_mode == "fp16x2" and released.coarse_mode == "fp16x2"        # the default generic answer is what it was
    for m, good, other in ((generic, ("generic_fp16x2", "generic"), ("fp16x2", "fp16")),
                           (released, ("fp16", "fp16x2"), ("generic", "generic_fp16x2"))):
        for name in ("nope", "", None, 17):
            with pytest.raises(ValueError):
                m.set_coarse_mode(name)
        for name in other:
            with pytest.raises(NotImplementedError):
                m.set_coarse_mode(name)
        assert "_coarse_mode" not in m.__dict__                    # nothing changed so far
        for name in good:                                          # nothing is packed: the choice is recorded for the next pack
            m.set_coarse_mode(name)
            assert m.coarse_mode == name


@pytest.mark.parametrize("case", nm.HIDDEN_CASES)
def test_added_inputs_are_what_they_claim(case):
    """The outlier channel leaves nr.MIN_SHARE of "big" alive (fp64 alone); up / down move the hidden volume by 2^+-10; the mixed
    batch's pairs differ by 2^12 in magnitude; every pair of every added input has a non-zero fp64 maximum."""
    ch = nm.outlier_channel(case)
    assert 0 <= ch < nr.CASES[case]["channels"][0]
    assert float((nm.expected(case, "big", "outlier")[1] > 0).double().mean()) >= nr.MIN_SHARE
    w, wu = nr.weights(case), nm.weights(case, "up")
    assert torch.equal(wu["conv.0.weight"], w["conv.0.weight"] * 1024) and torch.equal(wu["conv.2.weight"], w["conv.2.weight"])
    assert torch.equal(nm.weights(case, "down")["conv.0.bias"], w["conv.0.bias"] / 1024)
    x, y = nm.mixed(case)
    assert torch.equal(x[1], nr.volume("big")[1] * 4096) and torch.equal(x[2], nr.volume("big")[2] / 4096)
    assert all(y[z].abs().max() > 0 for z in range(3))
    assert nm.VOLUMES[nm.TILE][2] > 4 and nm.VOLUMES[nm.TILE][3] > 4 and nm.VOLUMES[nm.TILE][4] > 16
    for variant in (None,) + nm.VARIANTS:
        assert all(v.abs().max() > 0 for v in nm.expected(case, nm.TILE, variant)[1])


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    cxx = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    emu = os.path.join(ROOT, "tests", "hipemu")
    exe = str(tmp_path_factory.mktemp("ncn_pack") / "ncn_pack_dump")
    cmd = [cxx, "-std=c++17", "-O1", "-I", emu, os.path.join(ROOT, "tests", "ncn_pack_dump.cpp"), os.path.join(emu, "hipemu.cpp"),
           "-pthread", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


@pytest.mark.parametrize("k,co,ci,nh", [(3, 1, 16, 2), (5, 16, 16, 2), (3, 10, 7, 1), (3, 3, 4, 1), (5, 1, 10, 2)])
def test_plane_packing_against_its_definition(k, co, ci, nh, pack_program, tmp_path):
    gen = torch.Generator().manual_seed(100 * k + co + ci)
    w = torch.randn(k, co, ci, k, k, k, generator=gen) * torch.logspace(-3, 2, co).view(1, co, 1, 1, 1, 1)
    w[0, 0, 0, 0, 0, 0] = 0.0
    wn = w.numpy()
    ntap, tpm = k ** 3, 4 // nh
    nstep = (ntap + tpm - 1) // tpm
    seen = {}
    for br in (0, 1):
        src, dst = str(tmp_path / f"in{br}.bin"), str(tmp_path / f"out{br}.bin")
        with open(src, "wb") as f:
            f.write(np.array([k, co, ci, nh, br], dtype=np.int32).tobytes() + wn.tobytes())
        res = subprocess.run([pack_program, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert res.returncode == 0 and "ncn_pack_dump: ok" in res.stdout, res.stdout
        raw = open(dst, "rb").read()
        texp = np.frombuffer(raw[:4 * co], dtype=np.int32)
        planes = np.frombuffer(raw[4 * co:], dtype=np.float16).astype(np.float64).reshape(k, nstep, 2, 64, 8)
        # the exponent of a channel brings its largest |w| into [2^11, 2^12)
        for n in range(co):
            top = np.abs(wn[:, n]).max() * 2.0 ** int(texp[n])
            assert 2048 <= top < 4096, (n, top)
        # in the volume's own coordinates the transposed branch's weight of (da, db, dc, dd) is w[dc][dd][da][db]
        wb = wn if br == 0 else wn.transpose(4, 1, 2, 5, 0, 3)          # [da][o][i][db][dc][dd] of the branch
        want = np.zeros((k, nstep, 64, 8))
        for lane in range(64):
            n, g = lane & 15, lane >> 4
            for s in range(nstep):
                tap = tpm * s + g // nh
                for i in range(8):
                    ch = 8 * (g % nh) + i
                    if n < co and ch < ci and tap < ntap:
                        want[:, s, lane, i] = wb[:, n, ch, tap // (k * k), (tap // k) % k, tap % k].astype(np.float64) * 2.0 ** int(texp[n])
        got = planes[:, :, 0] + planes[:, :, 1]
        # hi + lo = the scaled weight to 2^-22 relative, or to half the spacing of fp16's subnormals (2^-25 under the scale that
        # puts the channel's largest weight at 2^11 or above: 2^-36 of it) where the low plane falls below fp16's normal range
        assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want) + 2.0 ** -25), np.abs(got - want).max()
        assert np.all(planes[:, :, 1][want == 0] == 0) and np.all(planes[:, :, 0][want == 0] == 0)       # the padding is zeros
        assert np.all(np.abs(planes[:, :, 1]) <= 2.0 ** -11 * np.abs(planes[:, :, 0]) + 2.0 ** -25)        # low plane: the residual
        seen[br] = (texp.copy(), planes)
    assert np.array_equal(seen[0][0], seen[1][0])                                                          # one exponent per channel, both branches
    assert not np.array_equal(seen[0][1], seen[1][1])
