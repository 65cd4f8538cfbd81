"""The host side of the cxx mixed-owner batches (the hb_cxx_prove_mixed /
hb_cxx_verify_rhs_mixed arena layouts and cost functions in
heartbeat_amd/csrc/hb_mixed_host.hpp, planned by hb_cbatch_plan): a stand-alone
program (tests/cxx_mixed_host/host_main.cpp) built with AddressSanitizer and
UBSan walks, over randomised mixes of primes, sector counts, key lengths, v_max
widths and challenge lengths, every group's arena against the items' exact
costs (total <= costs + 16 x sections), the ragged column / alpha-slot prefix
sums, the workgroup tables, the wave-job queue (every evaluation exactly once,
longest tries first) and that every item lands in exactly one group or in the
fall-through list."""
import os
import subprocess

from conftest import ROOT


def test_cxx_mixed_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx_mixed_host", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
