"""The prime kernels' lane code (heartbeat_amd/csrc/hb_prime.hpp) on the CPU:
a stand-alone program (tests/primeemul/main.cpp) built with AddressSanitizer
and UBSan runs hb_sprp_lane<NL> for every limb class over the shared vector
set (tests/prime_vectors.py: the bit lengths at the limb-class edges, 2^k +- 1,
k 2^m + 1 with large m, all-ones limbs, 2047, 3215031751, 561, squares and
products of recorded primes, small values in the widest class; bases 2, n - 2
and seeded ones) and hb_sieve_first_k, and the results are compared with
Python references written with pow() and %."""
import os
import random
import subprocess

import pytest

import prime_vectors as pv
from conftest import ROOT


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("primeemul") / "primeemul")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "primeemul", "main.cpp"), "-o", exe])

    def run(lines, tmp_path):
        path = str(tmp_path / "vectors.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == len(lines)
        return out
    return run


def test_sprp_lane_matches_pow(emul, tmp_path):
    lines, want, what = [], [], []
    for idx, (width, n, bases) in enumerate(pv.vectors()):
        nl = pv.nl_of_width(width)
        # the scan bound: the candidate's own length, or the class's
        maxbits = n.bit_length() if idx % 2 else 32 * nl
        for a in bases:
            for base2 in ((0, 1) if a == 2 else (0,)):
                lines.append("T %d %x %x %d %d" % (nl, n, a, base2, maxbits))
                want.append(int(pv.sprp(n, a)))
                what.append((nl, hex(n), hex(a), base2, maxbits))
    got = emul(lines, tmp_path)
    bad = [(w, g, e) for w, g, e in zip(what, got, want) if g != e]
    assert not bad, bad[:5]
    assert {w[0] for w in what} == {2, 8, 16, 32, 64}
    assert sum(want) > 50 and want.count(0) > 50      # both verdicts well covered
    # the named cases: 2047 and 3215031751 pass base 2, 561 passes none
    by = {(int(w[1], 16), int(w[2], 16)): g for w, g in zip(what, got)}
    assert by[(2047, 2)] == 1 and by[(3215031751, 2)] == 1 and by[(561, 2)] == 0
    assert by[(65537, 2)] == 1 and by[((1 << 32) + 1, 2)] == int(pv.sprp((1 << 32) + 1, 2))


def test_sprp_lane_3215031751_bases_2_3_5_7(emul, tmp_path):
    n = 3215031751
    got = emul(["T 2 %x %x 0 32" % (n, a) for a in (2, 3, 5, 7, 11)], tmp_path)
    assert got == [1, 1, 1, 1, 0] == [int(pv.sprp(n, a)) for a in (2, 3, 5, 7, 11)]


def test_sieve_first_k(emul, tmp_path):
    rng = random.Random(7)
    qs = [3, 5, 7, 251, 257, 65521, 65519] + [q for q in pv._SMALL if q > 1000][:5]
    lines, want = [], []
    for nl, bits in ((2, 8), (2, 64), (8, 129), (16, 512), (32, 1000), (32, 1024), (64, 2048)):
        for _ in range(3):
            start = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
            for q in qs:
                lines.append("K %d %x %d" % (nl, start, q))
                k = next(k for k in range(q) if (start + 2 * k) % q == 0)
                want.append(k)
    # a start that is a multiple of q, and one that is q itself
    for start, q in ((3 * 65521, 65521), (251, 251), (129, 131)):
        lines.append("K 2 %x %d" % (start, q))
        want.append(next(k for k in range(q) if (start + 2 * k) % q == 0))
    assert emul(lines, tmp_path) == want
