"""patch2pix_amd/csrc/host_pack.h on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: the stand-alone program
tests/hipemu/host_pack_test.cpp (its own main; no kernel is launched, nothing is loaded into python) is compiled against the
HIP stand-in, linked with tests/hipemu/hipemu.cpp and run.  It checks the blob's layout, upload, move and release rules, the
refused allocation (P2P_ENOMEM, a message, nothing leaked) and the shared arithmetic against restatements; the sanitizers turn
a leak, an overrun or undefined behaviour into a non-zero exit status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu")
CXX = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_pack") / "host_pack_test")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", EMU, os.path.join(EMU, "host_pack_test.cpp"),
           os.path.join(EMU, "hipemu.cpp"), "-pthread", "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode and "libclang_rt." in res.stdout:      # the link step cannot find the sanitizer runtime: no unsanitized build instead
        pytest.skip("the sanitizer runtime is missing: " + res.stdout.strip()[-400:])
    assert res.returncode == 0, res.stdout
    return exe


def test_host_pack_program_runs_clean_under_the_sanitizers(program):
    res = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "host_pack_test: ok" in res.stdout, res.stdout
    assert "runtime error" not in res.stdout and "ERROR: " not in res.stdout, res.stdout
