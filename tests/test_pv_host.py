"""The pure host header of the batched prove and verify calls
(heartbeat_amd/csrc/hb_pv_host.hpp): a stand-alone program
(tests/pv_host/host_main.cpp) built with AddressSanitizer and UBSan runs the
table fills of the eight calls -- schedules, staged files and tags, load16,
mu, wave-job queues -- against a transcription of the four fill loops they
replaced, over a staging buffer of exactly a group's size: the whole uploaded
range byte for byte, the device addresses of data and tags, every load16 flag,
the end cursor and the job count, for NL = 8 and NL = 32."""
import os
import subprocess

from conftest import ROOT


def test_pv_host_cases(tmp_path):
    exe = str(tmp_path / "host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pv_host", "host_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 10000, r.stdout
