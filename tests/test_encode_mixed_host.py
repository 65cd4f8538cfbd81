"""The pure host header of the mixed-owner encodes
(heartbeat_amd/csrc/hb_emixed_host.hpp): a stand-alone program
(tests/emixed_host/host_main.cpp) built with AddressSanitizer and UBSan walks,
over randomised mixes of primes, sector counts from 1 to T + 1, key lengths and
file lengths (empty files, thousands of files), every group's arena against the
files' costs (total <= costs + 16 x sections), the alpha-slot prefix sums and
F-buffer bases, the wave-job table (every evaluation exactly once, a file's
alpha wave-jobs directly before its F wave-jobs) and both workgroup tables with
a host model of the kernels' index arithmetic (every block tagged exactly once
by the launch of its shape, every alpha slot converted exactly once)."""
import os
import subprocess

from conftest import ROOT


def test_encode_mixed_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emixed_host", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
