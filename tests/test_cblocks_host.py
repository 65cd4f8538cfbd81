"""The pure host header of the cxx listed-block encode
(heartbeat_amd/csrc/hb_cblocks_host.hpp): a stand-alone program
(tests/cblocks_emul/main.cpp) built with AddressSanitizer and UBSan walks the
index-range check and its place after the descriptor checks, the split of the
lists into segments and groups under forced block and byte caps, the MAC count
of a segment whose last block is empty, each group's queue of wave-jobs, and
the fill of a group's staging buffer -- key schedules, records, wave-jobs, MAC
workgroups, narrowed indices, host blocks -- over a heap block of exactly the
uploaded size, for NL = 8, 32 and 64 and the three key lengths."""
import os
import subprocess

from conftest import ROOT


def test_cblocks_host_cases(tmp_path):
    exe = str(tmp_path / "cblocks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cblocks_emul", "main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
