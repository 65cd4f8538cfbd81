"""The pure host header of the batched calls (heartbeat_amd/csrc/hb_batch_host.hpp):
a stand-alone program (tests/batch_host/host_main.cpp) built with
AddressSanitizer and UBSan walks the six calls' arena layouts against their
cost functions (offsets multiples of 16, sections in order, up_bytes, total <=
costs + 16 x sections, sizes near 2^32 and at HB_BATCH_BYTES), the shared
grouping against a transcription of the greedy loop it replaced, and
be_to_limbs / to_be against the hand loops they replaced."""
import os
import subprocess

from conftest import ROOT


def test_batch_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "batch_host", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
