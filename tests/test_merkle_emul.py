"""The Merkle scheme's lane code (heartbeat_amd/csrc/hb_merkle.hpp) and the
host seed chain (hb_merkle_host.hpp) on the CPU: a stand-alone program
(tests/merkle_emul/main.cpp) built with AddressSanitizer and UBSan runs the
chain link, the leaf hash, the node hash of 0, 1 and 2 children and whole
small trees, and the results are compared with hmac / hashlib, the host
MerkleTree and the reference's recorded outputs
(tests/golden/merkle_scheme_cases.json)."""
import base64
import hashlib
import hmac
import os
import subprocess

import pytest

import merkle_golden as mg
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("merkle_emul")
    exe = str(d / "merkle_emul")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           # the runtimes inside the program: nothing is preloaded
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "heartbeat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "merkle_emul", "main.cpp"), "-o", exe])
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
    return load_golden("merkle_scheme_cases.json")


def _hx(b):
    return b.hex() if b else "-"


def _chain(key, seed, n):
    out, s = [], seed
    for _ in range(n):
        s = hmac.new(key, s, hashlib.sha256).digest()
        out.append(s)
    return out


def test_chain_matches_hmac(emul):
    """Keys of 0 (get_public's b''), 1, 16, 32, 63, 64, 65 (hashed first) and
    70 bytes; seeds of 0, 5, 32, 55, 56, 64 and 200 bytes (the first link is a
    generic HMAC); the lane chain and mk_host_chain agree (checked inside)."""
    keys = [b"", b"k", b"K" * 16, bytes(range(32)), b"x" * 63, b"y" * 64, b"z" * 65, bytes(range(70))]
    seeds = [b"", b"seed5", bytes(range(32, 64)), b"s" * 55, b"s" * 56, b"s" * 64, b"t" * 200]
    jobs = [(k, s, n) for k in keys for s, n in zip(seeds, (1, 2, 3, 5, 9, 17, 4))]
    got = emul(["L %s %s %d" % (_hx(k), _hx(s), n) for k, s, n in jobs])
    for (k, s, n), g in zip(jobs, got):
        assert g == b"".join(_chain(k, s, n)).hex(), (k, s, n)


def test_chain_matches_golden(emul, G):
    for c in G["cases"]:
        key, seed = bytes.fromhex(c["key"]), bytes.fromhex(c["seed"])
        got = bytes.fromhex(emul(["L %s %s %d" % (_hx(key), _hx(seed), c["n"])])[0])
        chals = [{"index": i, "seed": base64.b64encode(got[32 * i:32 * i + 32]).decode()} for i in range(c["n"])]
        assert mg.challenges_match(c, chals), (c["file"], c["n"])


def test_leaf_hash(emul):
    """Indices of 1 to 10 digits (the pad byte lands in every position of a
    word) against hashlib."""
    blob = hashlib.sha256(b"blob").digest()
    idx = [0, 9, 10, 99, 100, 256, 999, 1000, 9999, 10000, 65535, 65536, 99999, 123456, 4294967295]
    got = emul(["H %s %d" % (blob.hex(), i) for i in idx])
    assert got == [hashlib.sha256(blob + str(i).encode()).hexdigest() for i in idx]


def test_node_hash_0_32_64(emul):
    a, b = hashlib.sha256(b"a").digest(), hashlib.sha256(b"b").digest()
    got = emul(["N - - 0", "N %s - 1" % a.hex(), "N %s %s 2" % (a.hex(), b.hex())])
    assert got == [hashlib.sha256(b"").hexdigest(), hashlib.sha256(a).hexdigest(),
                   hashlib.sha256(a + b).hexdigest()]


def test_order(emul):
    ns = [1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 65535, 65536, 65537, (1 << 29), (1 << 29) + 1]
    got = emul(["O %d" % n for n in ns])
    assert [int(x) for x in got] == [0 if n == 1 else (n - 1).bit_length() for n in ns]


def test_plan_checks_and_ranges(emul):
    """The host's descriptor checks (made before any launch) and the PRF shape
    of a file's range, against KeyedPRF's own arithmetic (util.py:66-81)."""
    top = (1 << 64) - 1
    good = [(1, 100, 10, 100), (256, 1 << 20, 8192, 1 << 20), (3, 5, 8192, 5), (65536, 100003, 1, 200000),
            (5, 0, 8192, 0), (2, 255, 0, 255), (2, 256, 1, 256), (9, 1 << 32, 1, 1 << 33), (4, top, 1, top),
            (4, top - 1, 0, top)]
    bad = [((0, 100, 10, 100), -1), ((65537, 100, 10, 100), -1), ((4, 101, 10, 100), -1), ((4, top, 0, top), -4)]
    got = emul(["P %d %d %d %d" % g for g in good] + ["P %d %d %d %d" % b for b, _ in bad])
    for (n, filesz, chunksz, _), g in zip(good, got):
        chunk = min(chunksz, filesz)
        rng = filesz - chunk + 1
        nb = (rng.bit_length() + 7) // 8
        topmask = ((1 << rng.bit_length()) - 1) >> (8 * (nb - 1))
        order = (n - 1).bit_length()
        assert g == "%d:%d:%d:%d:%d:%d:%d" % (chunk, rng, nb, topmask, order, n, 2 << order), (n, filesz, chunksz)
    assert got[len(good):] == ["E%d" % code for _, code in bad]


def test_portable_compress_is_the_lane_compress(emul):
    assert emul(["C 64"]) == ["1"]


def test_small_trees_match_host_tree(emul):
    """Every n from 1 to 20 and 33: the lane tree's nodes are the host
    MerkleTree's, empty slots where it has b''."""
    from heartbeat_amd.Merkle.MerkleTree import MerkleTree
    ns = list(range(1, 21)) + [33]
    blobs = [hashlib.sha256(b"leaf%d" % k).digest() for k in range(max(ns))]
    got = emul(["T %d %s" % (n, " ".join(b.hex() for b in blobs[:n])) for n in ns])
    for n, g in zip(ns, got):
        t = MerkleTree()
        for b in blobs[:n]:
            t.add_leaf(b)
        t.build()
        assert len(t.nodes) == 2 << t.order
        assert g == b"".join(x if x else bytes(32) for x in t.nodes).hex(), n


def test_trees_match_golden(emul, G, oracle):
    """Every golden case of up to 65 leaves (the program takes the leaves on
    one line): the lane tree is the reference's stripped tree."""
    for c in G["cases"]:
        if c["n"] > 65:
            continue
        got = bytes.fromhex(emul(["T %d %s" % (c["n"], " ".join(x.hex() for x in mg.leaves_of(c, oracle)))])[0])
        order = (c["n"] - 1).bit_length()
        first_empty = (1 << order) - 1 + c["n"]
        assert len(got) == (2 << order) * 32 and not any(got[32 * first_empty:])
        nodes = [base64.b64encode(got[32 * k:32 * k + 32] if k < first_empty else b"").decode()
                 for k in range(2 << order)]
        tag = {"tree": {"nodes": nodes, "order": order, "leaves": []},
               "chunksz": c["tag"]["chunksz"], "filesz": c["tag"]["filesz"]}
        assert mg.tag_matches(c, tag), (c["file"], c["n"])
