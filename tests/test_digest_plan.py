"""The digest table's policy (heartbeat_amd/csrc/hb_digest_cache.hpp,
hb_digest_plan): a stand-alone program (tests/digest/plan_main.cpp) built with
AddressSanitizer and UBSan walks it through a request contained in the valid
range, touching, overlapping and disjoint ranges, a union over the cap, a
request over the cap, cap 0, an empty valid range and ranges near 2^64."""
import os
import subprocess

from conftest import ROOT


def test_digest_plan_cases(tmp_path):
    exe = str(tmp_path / "plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "digest", "plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 30, r.stdout
