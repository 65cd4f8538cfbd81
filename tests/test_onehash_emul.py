"""The OneHash scheme's lane code (heartbeat_amd/csrc/hb_onehash.hpp) and host
side (hb_onehash_host.hpp) on the CPU: a stand-alone program
(tests/onehash_emul/main.cpp) built with AddressSanitizer and UBSan runs the
plan rule, the segment hash and the chain link over heap buffers of the
file's exact size -- a whole-block load past the end is then a sanitizer
error -- and the descriptor checks of both entry points.  The results are
compared with the reference's recorded outputs
(tests/golden/onehash_cases.json) and with hashlib."""
import hashlib
import os
import subprocess

import pytest

import onehash_golden as og
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("onehash_emul")
    exe = str(d / "onehash_emul")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "onehash_emul", "main.cpp"), "-o", exe])
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


@pytest.fixture(scope="module")
def G():
    return load_golden("onehash_cases.json")


@pytest.fixture(scope="module")
def paths(tmp_path_factory, G):
    return og.write_files(tmp_path_factory.mktemp("onehash_files"), G["files"])


def _hx(b):
    return b.hex() if b else "-"


def _chain(s0, secret, n):
    out, s = [], s0
    for _ in range(n):
        out.append(s)
        s = hashlib.sha256(s + secret).digest()
    return out


def _plan(fs, block):
    """The issue's rule, restated: (off0, len0, off1, len1)."""
    c = min(1024, fs // 10)
    if block <= fs - c:
        return (block, c, 0, 0)
    a = block - (fs - c)
    return (block, min(block + a, fs) - block, 0, c - a)


def test_plan_rule(emul):
    """Every block of small files, and round the boundaries of large ones."""
    jobs = [(fs, b) for fs in (0, 1, 9, 10, 11, 19, 20, 100, 1000) for b in range(max(fs, 1))]
    for fs in (10239, 10240, 10241, 20000, 100003, (1 << 33) + 5):
        c = min(1024, fs // 10)
        jobs += [(fs, b) for b in (0, 1, fs - c - 1, fs - c, fs - c + 1, fs - c + c // 2, fs - c + c // 2 + 1,
                                   fs - 2, fs - 1)]
    got = emul(["P %d %d" % j for j in jobs])
    for (fs, b), g in zip(jobs, got):
        assert tuple(int(x) for x in g.split(":")) == _plan(fs, b), (fs, b)


def test_responses_match_golden(emul, G, paths):
    """Every in-range golden block with every seed of up to 64 bytes, at four
    alignments of the file and through the gather (compared inside)."""
    lines, want = [], []
    for name in G["files"]:
        lines.append("F %s" % paths[name])
        want.append(str(G["files"][name]["len"]))
        for c in G["meet"]:
            if c["file"] != name or c["part_len"] is None:
                continue
            for sl, resp in c["answers"].items():
                if int(sl) <= 64:
                    lines.append("R %d %s" % (c["block"], _hx(og.seed_of(int(sl)))))
                    want.append(resp)
    assert len(lines) > 900
    assert emul(lines) == want


def test_responses_match_hashlib(emul, tmp_path):
    """A file whose chunk is no multiple of 64 (c = 777): every block round the
    wrap and the short-read point, seeds of every length from 0 to 64 at one."""
    data = og.det_bytes("emul-file", 7777)
    p = tmp_path / "f.bin"
    p.write_bytes(data)
    fs, c = len(data), 777
    blocks = list(range(0, 70)) + list(range(fs - c - 70, fs - c + 70)) + \
        list(range(fs - c + c // 2 - 3, fs - c + c // 2 + 4)) + list(range(fs - 70, fs))
    jobs = [(b, og.seed_of(32)) for b in blocks] + [(fs - c + 5, og.seed_of(sl)) for sl in range(65)]
    got = emul(["F %s" % p] + ["R %d %s" % (b, _hx(s)) for b, s in jobs] + ["R %d -" % fs, "R %d -" % (fs + 1)])
    for (b, s), g in zip(jobs, got[1:]):
        o0, l0, o1, l1 = _plan(fs, b)
        assert g == hashlib.sha256(data[o0:o0 + l0] + data[o1:o1 + l1] + s).hexdigest(), (b, len(s))
    assert got[-2:] == ["E", "E"]


def test_chain_matches_hashlib_and_golden(emul, G):
    """Secrets of 0 to 24 bytes (one compression up to 23), 55, 56, 86, 87 (two)
    and 88, 200 (the host's generic link); then every golden chain."""
    s0 = hashlib.sha256(b"root").digest()
    secrets = [og.det_bytes("s%d" % n, n) for n in list(range(25)) + [55, 56, 86, 87, 88, 200]]
    got = emul(["L %s %s %d" % (s0.hex(), _hx(s), 5) for s in secrets] + ["L %s - 0" % s0.hex()])
    for s, g in zip(secrets, got):
        assert g == b"".join(_chain(s0, s, 5)).hex(), len(s)
    assert got[-1] == "-"
    cases = [c for c in G["generate"] if "seeds" in c and c["num"]]
    lines = []
    for c in cases:
        root = og.root_seed_of(c["root_seed"])
        first = hashlib.sha256(root if isinstance(root, bytes) else str(root).encode()).digest()
        lines.append("L %s %s %d" % (first.hex(), _hx(bytes.fromhex(c["secret"])), c["num"]))
    for c, g in zip(cases, emul(lines)):
        assert og.matches(c["seeds"], [g[64 * k:64 * k + 64] for k in range(c["num"])]), (c["file"], c["num"])


def test_descriptor_checks(emul):
    """Both entry points' checks, made before any launch: bad inputs are
    refused with the ABI's code, good ones planned."""
    gen = [("G 100 3 99 8 0", "3:0"), ("G 100 0 0 0 4", "0:0"), ("G 0 0 0 0 3", "0:0"), ("G 100 2 5 0 2", "2:0"),
           ("G 100 2 5 87 0", "2:0"), ("G 100 2 5 88 0", "2:2"),          # a long secret: the host's chain
           ("G 100 3 100 8 0", "E-1"), ("G 100 3 101 8 0", "E-1"), ("G 0 1 0 8 0", "E-1"),   # block >= len
           ("G 100 3 5 8 1", "E-1"), ("G 100 3 5 8 2", "E-1"), ("G 100 3 5 8 3", "E-1"),
           ("G 100 3 5 8 4", "E-1"), ("G 100 3 5 8 5", "E-1"),            # NULL buffers
           ("G 100 4294967296 5 8 4", "E-4")]                               # too many jobs
    meet = [("M 100 0 99 64 0", "120:02"), ("M 100 1 0 0 0", "201:01"),
            ("M 100 2 0 32 0", "E-1"),                                      # no such file
            ("M 100 0 100 32 0", "E-1"), ("M 0 0 0 32 0", "E-1"),           # block >= len
            ("M 100 0 5 65 0", "E-1"),                                      # seed too long
            ("M 100 0 5 32 1", "E-1"), ("M 100 0 5 32 2", "E-1"), ("M 100 0 5 32 3", "E-1"),
            ("M 100 0 5 32 4", "E-1")]
    up = [("U 1", str(8 << 20)), ("U 4096", str(8 << 20)), ("U 4097", str(2 * 4097 * 1024)),
          ("U %d" % (1 << 62), str((1 << 64) - 1))]
    cases = gen + meet + up
    assert emul([c for c, _ in cases]) == [w for _, w in cases]
