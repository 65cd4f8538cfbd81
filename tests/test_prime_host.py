"""The pure host header of hb_prime_search
(heartbeat_amd/csrc/hb_prime_host.hpp): a stand-alone program
(tests/primehost/host_main.cpp) built with AddressSanitizer and UBSan runs the
batch and selection logic against a simulated device (random base 2 and
full-round verdict tables): the result is the first survivor that passes
everything, no smaller survivor is ever left untested, the base 2 batches fill
the capacity without overshooting it (with 1, capacity and capacity + 1
starts), the window limit at the 2^bits edge, and the sieve's prime table."""
import os
import subprocess

from conftest import ROOT


def test_prime_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "primehost", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
