"""Where the matrix-core MACs read the file from
(heartbeat_amd/csrc/hb_mac_src.hpp): a stand-alone program
(tests/macsrc/addr_main.cpp) built with AddressSanitizer and UBSan sweeps file
lengths 0, 1, C - 1, C, C + 1, 64 C - 1 and 65 C + 17, S in {1, 2, 3, 4, 6, 16},
every lane of the last two waves and every K slice of the three 256-bit
layouts, and makes every 16-byte read on heap buffers of exactly the file's
and the fallback's sizes."""
import os
import subprocess

from conftest import ROOT


def test_mac_load_addresses(tmp_path):
    exe = str(tmp_path / "addr_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "macsrc", "addr_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 80000, r.stdout
