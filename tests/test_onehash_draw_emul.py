"""The OneHash draw's lane code (heartbeat_amd/csrc/hb_onehash_draw.hpp) and
the host checks of hb_onehash_pick_blocks_many and
hb_onehash_generate_drawn_many (hb_onehash_host.hpp) on the CPU: a stand-alone
program (tests/onehash_draw_emul/main.cpp) built with AddressSanitizer and
UBSan seeds, regenerates and draws over heap buffers of the exact sizes.  The
positions and the 625 state words are compared with Python's own ``random`` at
test time: random.seed(root), randint(0, len - 1) num times, random.getstate()."""
import os
import random
import subprocess

import pytest

import onehash_draw_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("onehash_draw_emul")
    exe = str(d / "onehash_draw_emul")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "onehash_draw_emul", "main.cpp"), "-o", exe])
    count = [0]

    def run(lines):
        count[0] += 1
        path = str(d / ("commands%d.txt" % count[0]))
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = r.stdout.split()
        assert len(out) == len(lines)
        return out
    return run


def _command(length, num, seed):
    return "D %d %d %s" % (length, num, ",".join("%x" % w for w in R.key_of(seed)))


def _token(blocks, words):
    return (",".join(str(b) for b in blocks) or "-") + ":" + "".join("%08x" % w for w in words)


def test_matrix_matches_random(emul):
    """Every range x seed x count: ranges of one value, round 2^32 (one word
    an attempt, then two) and up to 2^64 - 1; keys of 1 to 41 words; counts
    that stay in the first array and that cross one and two regenerations."""
    cases = R.matrix()
    assert len(cases) == 550
    got = emul([_command(*c) for c in cases])
    for (length, num, seed), g in zip(cases, got):
        assert g == _token(*R.expected(seed, length, num)), (length, num, seed)


def test_lazy_twist_boundary(emul):
    """A draw that consumes exactly 624 words ends on the first array with
    index 624, not on the second with 0; one more position regenerates."""
    length, num, seed = R.LAZY
    blocks, words = R.expected(seed, length, num)
    # the precondition, from the interpreter's own state: no attempt was rejected
    assert words[624] == 624
    random.seed(seed)
    first = [random.getrandbits(32) for _ in range(624)]
    assert blocks == [((first[2 * k + 1] >> 24) << 32) | first[2 * k] for k in range(num)]
    got = emul([_command(length, num, seed), _command(length, num + 1, seed), _command(length, num - 1, seed)])
    assert got[0] == _token(blocks, words)
    assert got[0].endswith("%08x" % 624)
    assert got[1] == _token(*R.expected(seed, length, num + 1)) and got[1].endswith("%08x" % 2)
    assert got[2] == _token(*R.expected(seed, length, num - 1)) and got[2].endswith("%08x" % 622)


def test_long_keys(emul):
    """Keys of 623 to 625 and of 1024 words: init_by_array walks max(624, len)
    steps and wraps the state index inside the key."""
    seeds = [(1 << (32 * 623)) - 1, (1 << (32 * 624)) - 1, (1 << (32 * 624)) + 12345, b"\x01" * 4032,
             bytes(4032)]   # leading zero bytes shorten the key
    assert [len(R.key_of(s)) for s in seeds] == [623, 624, 625, 1024, 16]
    got = emul([_command(1000, 5, s) for s in seeds])
    for s, g in zip(seeds, got):
        assert g == _token(*R.expected(s, 1000, 5)), len(R.key_of(s))


def test_descriptor_checks(emul):
    """Both entry points' checks, made before any launch: a bad descriptor is
    refused with the ABI's code, the message names its index, and nothing is
    planned; good ones are planned."""
    draw = [("C 100 3 5 0", "8:5:1"), ("C 1 1 7 0", "10:3:1"), ("C 0 1 0 0", "3:3:1"), ("C 100 1 0 2", "3:3:1"),
            ("C %d 1024 4 0" % ((1 << 64) - 1), "7:1026:1"),
            ("C 0 1 1 0", "E-1:1"),                                  # an empty range
            ("C 100 0 5 0", "E-1:1"), ("C 100 0 0 0", "E-1:1"),      # an empty key
            ("C 100 3 5 1", "E-1:1"), ("C 100 3 0 1", "E-1:1"),      # a NULL key
            ("C 100 3 5 2", "E-1:1"),                                # NULL blocks_out with num > 0
            ("C 100 1025 5 0", "E-4:1"), ("C 100 %d 5 0" % (1 << 40), "E-4:1"),   # a key above the cap
            ("C 100 3 %d 0" % ((1 << 31) - 2), "E-4:0"), ("C 100 3 %d 0" % (1 << 63), "E-4:0")]   # too many jobs
    gen = [("X 100 3 5 8 0", "8:5:0:0"), ("X 100 1 0 0 2", "3:3:0:0"), ("X 0 1 0 0 5", "3:3:0:0"),
           ("X 100 3 5 88 0", "8:5:0:2"),                            # a long secret: the host's chain
           ("X 0 1 1 8 0", "E-1:1"), ("X 100 0 5 8 0", "E-1:1"), ("X 100 3 5 8 1", "E-1:1"),
           ("X 100 3 5 8 2", "E-1:1"), ("X 100 3 5 8 3", "E-1:1"), ("X 100 3 5 8 4", "E-1:1"),
           ("X 100 3 5 8 5", "E-1:1"), ("X 100 3 5 8 6", "E-1:0"),
           ("X 100 1025 5 8 0", "E-4:1"), ("X 100 3 4294967296 8 0", "E-4:0")]
    cases = draw + gen
    assert emul([c for c, _ in cases]) == [w for _, w in cases]
