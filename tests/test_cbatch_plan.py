"""The planner of the batched cxx calls (heartbeat_amd/csrc/hb_cbatch_plan.hpp,
hb_cbatch_plan): a stand-alone program (tests/cbatch/plan_main.cpp) built with
AddressSanitizer and UBSan walks it through wave-job boundaries at HB_CB_JOB
+- 1, every evaluation covered exactly once, longest-first order over kinds of
unequal length, items without evaluations, the unit and byte caps with one
oversized item, fall-through, sizes near 2^64, and 500 random items."""
import os
import subprocess

from conftest import ROOT


def test_cbatch_plan_cases(tmp_path):
    exe = str(tmp_path / "plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cbatch", "plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 1000, r.stdout
