"""Regressor parity over dynamic range, on the kernels' own code executed on the CPU (tests/hipemu).

Every other regressor test draws its pyramids from one distribution (every pixel norm within a factor of two of every
other) and its checkpoint from one regime (BatchNorm weight 1 +- 0.1, running_var in [0.5, 1.5], weights of one
magnitude).  The fp16x2 paths carry their operands under SHARED power-of-two exponents (per image patch, per proposal,
per output channel), which those inputs never stretch.  Here: the stress families of tests/stress_inputs.py through
p2p_regress_batch, mid -> fine, against orc.fine_level evaluated in fp64, at the project's bars (coordinates 1e-3 px,
scores 1e-5) plus finite, in-bounds outputs; 48 x 64 pyramids, three proposals per case (an image corner, one across
the edge of the scaled region, one inside the dead region).  Modes fp16x2w and fp16x2 everywhere, f32 where the case
table (tests/range_reference.py) says so.  The fine level is fed the kernel's own mid matches.

contrast and reparam are asserted at the bars up to 2^16; at 2^20, 2^24 and 2^28 they are REPORTED (one printed line
per case and mode, pytest -s) and asserted only against the cap range_reference.cap derives.  Two cases go beyond the
families' list because a mutation of the kernel showed that nothing else reaches the code: global+30 (a pixel norm past
2^31: cell exponents below 100) and reparam_all24 (every |H| of a proposal far below 1).

Mutations this file turns red while the older emulated regressor tests stay green (run on scratch copies):
the cell-exponent clamp 13 / 240 narrowed to 100 / 140 (global+30); BN2 applied after the max instead of before it
(neg_gamma); the cell exponent taken from the largest per-pixel scale instead of the smallest (contrast_half16); the
max |H| reduction started at 1.0 instead of 0 (reparam_all24).

Cost.  A proposal and level is ~10 CPU-seconds in the emulator, a case and mode ~20 s of wall time on its three
emulated compute units, and there are 75 of them: about 90 CPU-MINUTES for the file (measured: 89), three times the
budget its issue hoped for -- the case list is the issue's, its estimate of 3 s per proposal and level was low.  So the
module fixture hands the selected cases to worker processes (this file run as a script, one per three cores of at most
16, at most eight workers) and the tests read their figures: 14 minutes of wall time with two workers on 8 cores.
Under pytest-xdist every xdist worker would start the whole job set of its own; run this file in one process."""
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))

H, W, N = 48, 64, 3
BASE_MODES = ("fp16x2w", "fp16x2")


def _run_job(emu, name, mode):
    """One case in one mode -> rr.measure's figures (assertions of rr.measure included)."""
    import emu_lib
    import golden_util as gu
    import range_reference as rr
    props = rr.proposals(H, W, N)
    if name in rr.PYRAMIDS:
        p1, p2 = rr.pair(name, H, W)
        sd = gu.state_dict(0)
    else:
        p1, p2 = rr.pair("plain", H, W)
        sd = rr.checkpoint(name, p1, p2, props)
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    mid = emu_lib.regressor_create(emu, sub("regress_mid."), mode)
    fine = emu_lib.regressor_create(emu, sub("regress_fine."), mode)
    try:
        out = emu_lib.regress(emu, mid, fine, p1, p2, props)
    finally:
        emu.p2p_regressor_destroy(mid)
        emu.p2p_regressor_destroy(fine)
    return rr.measure(out, sd, p1, p2, props, with_f32=True)


def _worker(out_file, jobs):
    import emu_lib
    emu = emu_lib.load()
    done = {}
    for job in jobs:
        name, mode = job.split(":")
        try:
            done[job] = _run_job(emu, name, mode)
        except Exception as e:                                   # an assertion of rr.measure or an error of the library
            done[job] = {"error": f"{type(e).__name__}: {e}"}
        with open(out_file, "w") as f:
            json.dump(done, f)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    _worker(sys.argv[1], sys.argv[2:])
    sys.exit(0)

import golden_util as gu  # noqa: E402
import range_reference as rr  # noqa: E402


@pytest.fixture(scope="module")
def figures(request, tmp_path_factory):
    """{"name:mode": figures} of every selected case of this module, computed by worker processes."""
    import build_emu
    build_emu.build()                                            # once, before the workers need it
    jobs = sorted({f"{it.callspec.params['name']}:{it.callspec.params['mode']}" for it in request.session.items
                   if getattr(it, "module", None) is request.module and hasattr(it, "callspec") and "mode" in it.callspec.params})
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 3)
    nw = max(1, min(8, (min(cores, 16) + 1) // 3, len(jobs)))
    tmp = tmp_path_factory.mktemp("range_emu")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE] + sys.path))
    procs = []
    for w in range(nw):
        f = str(tmp / f"worker{w}.json")
        procs.append((f, subprocess.Popen([sys.executable, os.path.abspath(__file__), f] + jobs[w::nw], env=env, cwd=os.path.dirname(HERE))))
    out = {}
    for f, p in procs:
        p.wait()
        if os.path.exists(f):
            with open(f) as fh:
                out.update(json.load(fh))
    return out


def _figures_of(figures, name, mode):
    res = figures.get(f"{name}:{mode}")
    assert res is not None, f"the worker process of {name}:{mode} ended before it got there"
    assert "error" not in res, res["error"]
    print(f"\nrange[emulator] {name:>20s} {mode:>8s}: coord {res['coord']:.2e} px  score {res['score']:.2e}  raw {res['raw']:.2e}"
          f"  | fp32 oracle: {res['o32_coord']:.2e} px  {res['o32_score']:.2e}  {res['o32_raw']:.2e}")
    return res


def _modes(table, names):
    return [(n, m) for n in names for m in BASE_MODES + (("f32",) if table[n][-1] else ())]


@pytest.mark.parametrize("name,mode", _modes(rr.PYRAMIDS, rr.MANDATORY_PYRAMIDS))
def test_pyramid_families_at_the_bars(name, mode, figures):
    res = _figures_of(figures, name, mode)
    assert res["coord"] <= rr.COORD_TOL and res["score"] <= rr.SCORE_TOL, res


@pytest.mark.parametrize("ckpt", ["reparam8", "reparam16", "reparam28", "octaves"])
def test_exact_reparametrisations_do_not_move_the_reference(ckpt):
    """reparam and octaves rescale by powers of two on both sides of a linear step: the fp64 reference's raw outputs are
    the SAME BITS as with the plain checkpoint, so whatever a kernel loses on them is the kernel's."""
    p1, p2 = rr.pair("plain", H, W)
    props = rr.proposals(H, W, N)
    base = rr.reference64(gu.state_dict(0), p1, p2, props)
    got = rr.reference64(rr.checkpoint(ckpt, p1, p2, props), p1, p2, props)
    assert torch.equal(got[2], base[2]) and torch.equal(got[0], base[0])


@pytest.mark.parametrize("name,mode", _modes(rr.CHECKPOINTS, rr.MANDATORY_CHECKPOINTS))
def test_checkpoint_families_at_the_bars(name, mode, figures):
    res = _figures_of(figures, name, mode)
    assert res["coord"] <= rr.COORD_TOL and res["score"] <= rr.SCORE_TOL, res


@pytest.mark.parametrize("name,mode", [(f"{fam}{k}", m) for fam in ("contrast_half", "reparam") for k in rr.REPORTED_OCTAVES
                                       for m in BASE_MODES + ("f32",)])
def test_reported_beyond_the_mandatory_line(name, mode, figures):
    """Reported, not asserted at the bars in the two-plane modes: finite, in-bounds outputs (rr.measure) and no more than
    cap(k) = 2^(k - 16) times the bars (derivation: range_reference.cap).  Mode f32 is the control: at the bars, for every
    k.  DESIGN.md, "Numeric domain of the fp16x2 paths", holds the table."""
    res = _figures_of(figures, name, mode)
    f = rr.reported_factor(int(name[-2:]), mode)
    assert res["coord"] <= rr.COORD_TOL * f and res["score"] <= rr.SCORE_TOL * f, res
