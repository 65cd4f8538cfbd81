"""GPU parity of every encode MAC path on extreme files under edge primes.

The other GPU encode tests feed the sector MACs uniformly random bytes under
seeded random primes.  Here the primes are the largest below 2^b and the
smallest above 2^(b-1) (edge_primes.py: under them a sector is routinely not
below p, up to almost 2p) and the files are the inputs a multiply-accumulate
gets wrong in one case in 2^32:

* constant 0x00 (the one asymmetric int8 value, -128, of the MFMA MACs; the
  tag is exactly F), 0xFF (+127; a sector >= p when bitlen(p) % 8 == 0), 0x80
  (every int8 product zero) and 0x7F,
* bytes alternating 0x00 / 0xFF, whole sectors alternating all-0xFF /
  all-0x00, whole blocks alternating all-0xFF / random,
* a one-hot sweep: block b is zero except byte b % C = 0x01, so that its tag
  is F_b + alpha_j 256^(ss-1-k) and a mismatch names the table entry,
* a file of solved blocks whose tags are 0 and p - 1 in turn (nul_file): the
  sum before the last reduction is an exact multiple of p, or one below it,

over 257 whole blocks plus a last block of 1 and of C - 1 bytes (a full
hb_wmac_kernel workgroup, a partial one and the tail kernel), C blocks + 1
byte for the sweep, block_base 0 and 2^32 - 30.

Every tag of every block is compared with two references: the CPU oracle
(oracle.encode / oracle.cxx_encode) and the definition in Python ints,
tag_i = (F(i) + sum_j alpha_j m_ij) % p with F and alpha from the oracle's PRF;
the all-zero file also against hb_prf_eval of the indices.  Both references
are computed once per (prime, S, file) and shared by the paths.

Paths and the switches that select them (the gate is open in conftest.py):
256-bit MFMA MACs (16x16x64, 32x32x32 whole lines, sector loads), the VALU
MAC, the small-encode launch, the cxx PRF, S = HB_MFMA_MAX_S and the fallback
past it; the byte-shaped sectors of 255-, 128-, 64- and 61-bit primes; the
split wide-prime MAC (hb_wide.hpp) at 512, 1024, 2048, 1020 and 1000 bits on
the two-pass engine, the mid-size path and against $HB_NO_WIDE, its per-lane
finish, C == HB_WIDE_MAX_C exactly and the fallback past it; and the five
batched entries.  Reference: PySwizzle.py:279-314, util.py:83-96.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import edge_primes as E
from test_gpu_blocks import blocks_many
from test_gpu_cxx_many import encode_many as cxx_encode_many
from test_gpu_encode_many import encode_many
from test_gpu_encode_mixed import encode_mixed
from test_gpu_parity import DevBuf

pytestmark = pytest.mark.gpu

BASE_HI = 2 ** 32 - 30
NFULL = 257
CONSTS = {"00": 0x00, "ff": 0xFF, "80": 0x80, "7f": 0x7F}
TWO_PASS = {"HB_NO_SMALL_ENCODE": "1"}
SWITCHES = ("HB_NO_SMALL_ENCODE", "HB_MFMA_MIN_S", "HB_MFMA_LINE32", "HB_NO_MFMA", "HB_NO_WIDE")


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


# ------------------------------------------------------------------ files
def make_file(pattern, n, ss, C, seed=0):
    """The bytes of one extreme file of n bytes (sectors of ss, blocks of C bytes)."""
    if pattern in CONSTS:
        return bytes([CONSTS[pattern]]) * n
    if pattern == "alt":        # bytes 0x00, 0xFF, 0x00, ...
        return (b"\x00\xff" * (n // 2 + 1))[:n]
    if pattern == "sec":        # sectors all-0xFF, all-0x00, ... (S odd: the phase flips per block)
        return ((b"\xff" * ss + b"\x00" * ss) * (n // (2 * ss) + 1))[:n]
    if pattern == "blk":        # blocks all-0xFF, random, all-0xFF, ...
        a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        for b in range(0, n // C + 1, 2):
            a[b * C:(b + 1) * C] = 0xFF
        return a.tobytes()
    if pattern == "hot":        # block b: byte b % C is 0x01, every other byte zero
        a = np.zeros(n, dtype=np.uint8)
        pos = np.arange(n // C + 1, dtype=np.int64) * C + np.arange(n // C + 1, dtype=np.int64) % C
        a[pos[pos < n]] = 1
        return a.tobytes()
    if pattern == "rnd":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    raise ValueError(pattern)


def nul_file(prf, p, S, fk, ak, n, base):
    """Blocks whose tags are 0 and p - 1 in turn: sector 0 of block i solves
    F(i) + alpha_0 m + alpha_1 t = 0 (i even) or -1 (i odd) mod p, the other
    sectors are zero.  The sum before the final reduction is then an exact
    multiple of p (the reduction must take the last p off: v == p) or one
    below it (it must not).  Where bitlen(p) % 8 != 0 a solution m seldom fits
    a sector: sector 1 = t counts up until one does (S = 1: such a block stays
    zero).  Returns (bytes, {block: tag})."""
    ss = p.bit_length() // 8
    C = ss * S
    inv = pow(prf(ak, 0), -1, p)
    a1 = prf(ak, 1) if S > 1 else 0
    buf, solved = bytearray(n), {}
    for i in range(n // C):
        target = 0 if i % 2 == 0 else p - 1
        rest = target - prf(fk, base + i)
        for t in range(2048 if S > 1 else 1):
            m = (rest - a1 * t) * inv % p
            if m < 256 ** ss:
                buf[i * C:i * C + ss] = m.to_bytes(ss, "big")
                if t:
                    buf[i * C + ss:i * C + 2 * ss] = t.to_bytes(ss, "big")
                solved[i] = target
                break
    return bytes(buf), solved


def file_list(C, patterns=None, nfull=NFULL, sweep=True):
    """[(label, pattern, length, block_base)]: every pattern with a last block
    of 1 byte at block_base 0 and of C - 1 bytes at 2^32 - 30, then the sweep
    and the file of solved blocks."""
    out = []
    for pat in patterns or (list(CONSTS) + ["alt", "sec", "blk"]):
        out.append(("%s+1" % pat, pat, nfull * C + 1, 0))
        out.append(("%s+C-1" % pat, pat, nfull * C + C - 1, BASE_HI))
    if sweep:
        out.append(("hot", "hot", C * C + 1, 0))
        out.append(("nul", "nul", nfull * C + 1, BASE_HI))
    return out


def keys_of(tag):
    return hashlib.sha256(b"xt-f-" + tag.encode()).digest(), hashlib.sha256(b"xt-a-" + tag.encode()).digest()


# ------------------------------------------------------------------ references
def prf_of(oracle, p, cxx):
    """prf(key, x) with range p: KeyedPRF.eval, or the cxx prf of the 32-bit index."""
    if cxx:
        return lambda k, x: oracle.cxx_prf_eval(k, p, x & 0xFFFFFFFF)[0]
    return lambda k, x: oracle.prf_eval(k, p, x)


def direct_tags(oracle, p, S, fk, ak, data, base, cxx=False):
    """tag_i = (F(i) + sum_j alpha_j m_ij) % p in Python ints; the sector loop
    stops after the first short read (PySwizzle.py:297-307).  cxx: the cxx
    prf of the 32-bit index, and a block that reads no sector keeps F as it is
    (shacham_waters_private.cxx:681-690)."""
    ss = p.bit_length() // 8
    C = ss * S
    prf = prf_of(oracle, p, cxx)
    alpha = [prf(ak, j) for j in range(S)]
    zero = bytes(ss)
    tags = []
    for i in range(len(data) // C + 1):
        acc = prf(fk, base + i)
        blk = data[i * C:(i + 1) * C]
        if cxx and not blk:
            tags.append(acc)
            continue
        for j in range(S):
            sec = blk[j * ss:(j + 1) * ss]
            if len(sec) == ss and sec == zero:
                continue
            if sec:
                acc += alpha[j] * int.from_bytes(sec, "big")
            if len(sec) != ss:
                break
        tags.append(acc % p)
    return tags


_REFS = {}


def references(oracle, p, S, label, pattern, n, base, cxx=False):
    """(keys, file bytes, tags) of one file: the tags are the oracle's, checked
    once against the Python-int definition (and the sweep's closed form)."""
    key = (p, S, label, n, base, cxx)
    if key not in _REFS:
        ss = p.bit_length() // 8
        C = ss * S
        fk, ak = keys_of("%x-%d-%s" % (p & 0xFFFFFFFFFFFF, S, label))
        solved = {}
        if pattern == "nul":
            data, solved = nul_file(prf_of(oracle, p, cxx), p, S, fk, ak, n, base)
            assert len(solved) == n // C or (S == 1 and p.bit_length() % 8)
        else:
            data = make_file(pattern, n, ss, C, seed=S * 1000 + p.bit_length())
        enc = oracle.cxx_encode if cxx else oracle.encode
        want = enc(p, S, fk, ak, data, block_base=base, nthreads=8)
        assert all(want[i] == t for i, t in solved.items()), (label, "a solved block's tag")
        assert want == direct_tags(oracle, p, S, fk, ak, data, base, cxx), (label, "the references disagree")
        if pattern == "hot" and not cxx:
            alpha = [oracle.prf_eval(ak, p, j) for j in range(S)]
            for b in range(n // C + 1):
                j, k = (b % C) // ss, (b % C) % ss
                e = ss - 1 - k if b < n // C else 0      # the last block's sector is 1 byte long
                assert want[b] == (oracle.prf_eval(fk, p, base + b) + alpha[j] * 256 ** e) % p, (b, j, k)
        _REFS[key] = (fk, ak, data, want)
    return _REFS[key]


def gpu_prf(nat, key, p, xs):
    ctx = nat.context()
    w = nat.width_of(p)
    arr = np.asarray(xs, dtype=np.uint64)
    out = ctypes.create_string_buffer(w * len(xs))
    pb = nat.be(p)
    with ctx.lock:
        ctx.check(nat.lib().hb_prf_eval(ctx.h, key, len(key), pb, len(pb), arr.ctypes.data, len(xs), out))
    return [int.from_bytes(out.raw[i * w:(i + 1) * w], "big") for i in range(len(xs))]


# ------------------------------------------------------------------ one encode
def run_encode(nat, p, S, fk, ak, data, base, cxx=False, toff=0):
    """Device-resident hb_encode (status 0 checked): (tags as ints, launches)."""
    ctx = nat.context()
    w = nat.width_of(p)
    nb = len(data) // ((p.bit_length() // 8) * S) + 1
    pb = nat.be(p)
    buf, tb = DevBuf(nat, max(len(data), 16)), DevBuf(nat, nb * w + 32)
    try:
        buf.upload(data)
        tb.upload(b"\xa5" * (nb * w + 32))
        flags = 3 | (nat.HB_PRF_CXX if cxx else 0)
        with ctx.lock:
            ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), base, buf.p, len(data), nb,
                                          tb.p + toff, flags, None))
        launches = ctx.last_kernel_ms()[1]
        raw = tb.download()
    finally:
        buf.free()
        tb.free()
    assert raw[:toff] == b"\xa5" * toff and raw[toff + nb * w:] == b"\xa5" * (32 - toff)
    return [int.from_bytes(raw[toff + i * w:toff + (i + 1) * w], "big") for i in range(nb)], launches


def set_switches(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def first_diff(got, want):
    assert len(got) == len(want)
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    return None if not bad else (bad[0], len(bad), hex(got[bad[0]]), hex(want[bad[0]]))


_SEEN = {}   # (p, S, label, cxx) -> tags of the first path that ran the file


def check_path(nat, oracle, monkeypatch, p, S, env, files, cxx=False, toff=0):
    """Every file of `files` through one path: tags == both references, == the
    paths that ran the same file before, all-zero file == hb_prf_eval(indices)."""
    set_switches(monkeypatch, env)
    launches = {}
    for label, pattern, n, base in files:
        fk, ak, data, want = references(oracle, p, S, label, pattern, n, base, cxx)
        got, launches[label] = run_encode(nat, p, S, fk, ak, data, base, cxx, toff)
        assert first_diff(got, want) is None, (p.bit_length(), S, sorted(env), label, first_diff(got, want))
        assert _SEEN.setdefault((p, S, label, cxx), got) == got
        if pattern == "00" and not cxx:
            assert got == gpu_prf(nat, fk, p, [base + i for i in range(len(got))]), label
    return launches


# ------------------------------------------------------------------ 256-bit paths
MFMA = dict(TWO_PASS, HB_MFMA_MIN_S="2")
PATHS_256 = [
    ("m16", 2, MFMA), ("m16", 6, MFMA), ("m16", 16, MFMA),              # 16x16x64
    ("line32", 4, dict(MFMA, HB_MFMA_LINE32="1")),                      # 32x32x32 whole lines
    ("sector", 3, MFMA), ("sector", 5, MFMA),                           # sector loads (S odd)
    ("valu", 1, dict(TWO_PASS, HB_NO_MFMA="1")), ("valu", 16, dict(TWO_PASS, HB_NO_MFMA="1")),
    ("small", 1, {}), ("small", 10, {}),                                # the small-encode launch
]


@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("name,S,env", PATHS_256, ids=["%s-S%d" % (n, s) for n, s, _ in PATHS_256])
def test_256bit_mac_paths(nat, oracle, monkeypatch, name, S, env, which):
    p = E.edge(256, which)
    check_path(nat, oracle, monkeypatch, p, S, env, file_list(32 * S))


@pytest.mark.parametrize("which", ["max", "min"])
def test_256bit_cxx_prf(nat, oracle, monkeypatch, which):
    p = E.edge(256, which)
    check_path(nat, oracle, monkeypatch, p, 10, {}, file_list(320), cxx=True)


@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("S", [2048, 2050])
def test_256bit_largest_mfma_block_and_fallback(nat, oracle, monkeypatch, S, which):
    """S = HB_MFMA_MAX_S (64 KiB blocks) on the MFMA MAC, S = 2050 on the VALU
    MAC that takes over past it: constant files of 33 blocks + 1 byte."""
    p = E.edge(256, which)
    files = [("%s+1" % pat, pat, 33 * 32 * S + 1, BASE_HI if k % 2 else 0) for k, pat in enumerate(CONSTS)]
    check_path(nat, oracle, monkeypatch, p, S, MFMA, files)


# ------------------------------------------------------------------ byte-shaped sectors, NL = 2
@pytest.mark.parametrize("engine", ["small", "two_pass"])
@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("S", [1, 4, 7])
@pytest.mark.parametrize("bits", [255, 128, 64, 61])
def test_narrow_primes(nat, oracle, monkeypatch, bits, S, which, engine):
    p = E.edge(bits, which)
    check_path(nat, oracle, monkeypatch, p, S, TWO_PASS if engine == "two_pass" else {}, file_list((bits // 8) * S))


# ------------------------------------------------------------------ split wide-prime MAC
WIDE_PATHS = {"two_pass": TWO_PASS, "mid": {}, "no_wide": dict(TWO_PASS, HB_NO_WIDE="1")}


@pytest.mark.parametrize("path", list(WIDE_PATHS))
@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("bits,S", [(512, 16), (1024, 10), (2048, 4)])
def test_wide_mac_paths(nat, oracle, monkeypatch, bits, S, which, path):
    """The split MAC on the two-pass engine and on the mid-size path, and the
    in-kernel VALU MAC ($HB_NO_WIDE): each == the references, and == each other
    through check_path's record of the earlier paths' tags."""
    p = E.edge(bits, which)
    check_path(nat, oracle, monkeypatch, p, S, WIDE_PATHS[path], file_list((bits // 8) * S))


@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("bits,S", [(1020, 16), (1000, 32)])
def test_wide_mac_narrow_tags(nat, oracle, monkeypatch, bits, S, which):
    """127-byte sectors, and 125-byte sectors with tw = 125: F in a buffer of
    its own, D = 125 digits, a partial last tile."""
    p = E.edge(bits, which)
    check_path(nat, oracle, monkeypatch, p, S, TWO_PASS, file_list((bits // 8) * S))


@pytest.mark.parametrize("which", ["max", "min"])
def test_wide_mac_per_lane_finish(nat, oracle, monkeypatch, which):
    """Tags at a 4-byte-offset address: hb_wmac_kernel's per-lane finish."""
    p = E.edge(1024, which)
    check_path(nat, oracle, monkeypatch, p, 10, TWO_PASS, file_list(1280), toff=4)


@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("bits,S", [(1024, 256), (2048, 128), (512, 512)])
def test_wide_mac_largest_block(nat, oracle, monkeypatch, bits, S, which):
    """C == HB_WIDE_MAX_C (32768) exactly, constants 0x00 and 0xFF (the int32
    column sums at their largest magnitude), 130 blocks + 1 byte: the split
    MAC runs (more launches than under $HB_NO_WIDE: the digit table and the
    MAC kernels) and equals the VALU MAC and the references."""
    p = E.edge(bits, which)
    C = (bits // 8) * S
    assert C == 32768
    files = [("00+1", "00", 130 * C + 1, 0), ("ff+1", "ff", 130 * C + 1, BASE_HI)]
    wide = check_path(nat, oracle, monkeypatch, p, S, TWO_PASS, files)
    check_path(nat, oracle, monkeypatch, p, S, {}, files)
    valu = check_path(nat, oracle, monkeypatch, p, S, WIDE_PATHS["no_wide"], files)
    assert wide["ff+1"] > valu["ff+1"], (wide, valu)


@pytest.mark.parametrize("which", ["max", "min"])
def test_wide_mac_declines_past_largest_block(nat, oracle, monkeypatch, which):
    """C = 32784 = 683 sectors of a 384-bit prime: wide_plan declines, the
    VALU MAC runs with and without $HB_NO_WIDE (the same launches)."""
    p = E.edge(384, which)
    S, C = 683, 32784
    files = [("00+1", "00", 130 * C + 1, 0), ("ff+1", "ff", 130 * C + 1, BASE_HI)]
    a = check_path(nat, oracle, monkeypatch, p, S, TWO_PASS, files)
    b = check_path(nat, oracle, monkeypatch, p, S, WIDE_PATHS["no_wide"], files)
    assert a == b


# ------------------------------------------------------------------ batches
BATCH_SHAPES = {256: 16, 1024: 10}                    # bits -> S
BATCH_PRIMES = [(256, "max"), (256, "min"), (1024, "max"), (1024, "min")]


def batch_files(oracle, p, S, cxx=False, tagged=""):
    """[(label, base, f_key, alpha_key, bytes, reference tags)]: 0x00, 0xFF,
    0x80 and sector-alternating files of 3 blocks + 1 byte and of 70 blocks,
    and one random file."""
    C = (p.bit_length() // 8) * S
    out = []
    for pat in ("00", "ff", "80", "sec"):
        for n in (3 * C + 1, 70 * C):
            label = "b%s-%s-%d" % (tagged, pat, n)
            out.append((label, 0) + references(oracle, p, S, label, pat, n, 0, cxx))
    label = "b%s-rnd" % tagged
    out.append((label, 0) + references(oracle, p, S, label, "rnd", 9 * C + 5, 0, cxx))
    return out


def raw_of(tags, w):
    return b"".join(t.to_bytes(w, "big") for t in tags)


def singles(nat, monkeypatch, p, S, files, cxx=False):
    """The loop of single encodes the batch replaces: each == the references."""
    set_switches(monkeypatch, {})
    for label, base, fk, ak, data, want in files:
        got, _ = run_encode(nat, p, S, fk, ak, data, base, cxx)
        assert got == want, (label, first_diff(got, want))


@pytest.mark.parametrize("bits,which", BATCH_PRIMES)
def test_encode_many(nat, oracle, monkeypatch, bits, which):
    p, S = E.edge(bits, which), BATCH_SHAPES[bits]
    files = batch_files(oracle, p, S)
    singles(nat, monkeypatch, p, S, files)
    rc, got, _ = encode_many(nat, p, S, [(f[2], f[3]) for f in files], [f[4] for f in files])
    assert rc == 0
    for f, g in zip(files, got):
        assert g == raw_of(f[5], nat.width_of(p)), f[0]


@pytest.mark.parametrize("bits,which", BATCH_PRIMES)
def test_cxx_encode_many(nat, oracle, monkeypatch, bits, which):
    p, S = E.edge(bits, which), BATCH_SHAPES[bits]
    files = batch_files(oracle, p, S, cxx=True)
    singles(nat, monkeypatch, p, S, files, cxx=True)
    rc, got, _ = cxx_encode_many(nat, p, S, [(f[2], f[3]) for f in files], [f[4] for f in files])
    assert rc == 0
    for f, g in zip(files, got):
        assert g == raw_of(f[5], nat.width_of(p)), f[0]


def mixed_items(oracle, rot, cxx):
    """Nine files, file k under prime (k + rot) % 4 of BATCH_PRIMES."""
    items, refs = [], []
    for k in range(9):
        bits, which = BATCH_PRIMES[(k + rot) % 4]
        p, S = E.edge(bits, which), BATCH_SHAPES[bits]
        f = batch_files(oracle, p, S, cxx, tagged="m")[k]
        items.append((p, S, f[2], f[3], f[4]))
        refs.append((p, S, f))
    return items, refs


@pytest.mark.parametrize("cxx", [False, True], ids=["hb_encode_mixed", "hb_cxx_encode_mixed"])
@pytest.mark.parametrize("rot", range(4))
def test_encode_mixed(nat, oracle, monkeypatch, rot, cxx):
    """Each file under its own prime, the max and min of 256 and 1024 bits in
    one call; over the four rotations every file meets every prime."""
    items, refs = mixed_items(oracle, rot, cxx)
    for p, S, f in refs:
        singles(nat, monkeypatch, p, S, [f], cxx)
    rc, got, _, _ = encode_mixed(nat, items, cxx=cxx)
    assert rc == 0
    for (p, S, f), g in zip(refs, got):
        assert g == raw_of(f[5], nat.width_of(p)), (f[0], p.bit_length())


@pytest.mark.parametrize("bits,which", BATCH_PRIMES)
def test_encode_blocks_many(nat, oracle, monkeypatch, bits, which):
    """The listed blocks are each file's own, in order, from block 0 (and from
    2^32 - 30 for every other file), so a single hb_encode of the range is the
    loop the call replaces."""
    p, S = E.edge(bits, which), BATCH_SHAPES[bits]
    C = (bits // 8) * S
    files = []
    for k, f in enumerate(batch_files(oracle, p, S)):
        label, _, _, _, data, _ = f
        base = BASE_HI if k % 2 else 0
        pat = "rnd" if label.endswith("rnd") else label.split("-")[1]
        files.append(("k" + label, base) + references(oracle, p, S, "k" + label, pat, len(data), base))
    singles(nat, monkeypatch, p, S, files)
    listed = [(f[2], f[3], [f[1] + i for i in range(len(f[4]) // C + 1)], f[4]) for f in files]
    rc, got, _ = blocks_many(nat, p, S, listed)
    assert rc == 0
    for f, g in zip(files, got):
        assert g == raw_of(f[5], nat.width_of(p)), f[0]
