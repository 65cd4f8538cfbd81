"""The pure host header of the mixed-owner batches
(heartbeat_amd/csrc/hb_mixed_host.hpp): a stand-alone program
(tests/mixed_host/host_main.cpp) built with AddressSanitizer and UBSan walks,
over randomised mixes of primes, sector counts, key lengths and challenge
lengths, the class partition (every item in exactly one class, input order
kept), every group's arena against the items' costs (total <= costs + 16 x
sections), the ragged column / alpha-slot prefix sums, the sum launch's and the
conversion pass's workgroup tables (every term exactly once, one proof per
workgroup) and the distinct-prime cache."""
import os
import subprocess

from conftest import ROOT


def test_mixed_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mixed_host", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
