"""GPU parity of the mixed-owner encode (hb_encode_mixed,
PySwizzle.encode_mixed): the tags of many files that each name their own prime,
sector count and key length, in one call: per group of a (limb count, AES round
count) class one PRF launch, one conversion pass and a MAC launch per shape
(hb_emixed.hpp; hb_runtime.cpp encode_mixed_impl).

Every comparison is byte for byte, every file of every batch: the mixed call
against hb_encode per file and against the CPU oracle's encode, and tries_out
against the sum of the single calls' tries.  Over

* one prime and one S (== hb_encode_many), neighbours that differ in modulus,
  geometry and S inside one group, in three orders,
* S at every MAC boundary (1, 2, 3, 16, 17, T - 1, T, T + 1, 255, 256, 257),
  file lengths at every boundary of the file's own geometry and files that
  cross a MAC workgroup,
* every limb class and key size in one call, the reference's recorded encodes
  (tests/golden/encode_cases.json) in one call,
* equal bytes and keys under different primes, one prime on non-adjacent files,
* device- and host-resident data and tags with differing 16-byte alignment
  between neighbours,
* group splitting and a large file's fall-through under its own prime, every
  rejected descriptor, unsupported flags, the context afterwards,
* PySwizzle.encode_mixed -> prove_mixed -> verify_mixed end to end.

The helpers take `cxx` so that tests/test_gpu_cxx_encode_mixed.py shares them.

Reference: a loop over PySwizzle.py:279-311 for many owners (one prime per
PySwizzle instance, :250-251)."""
import ctypes
import importlib
import io
import random

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import P256, DevBuf
from test_gpu_prove_many import P255, P256MAX, last_error, oracle_proof, prove_single

pytestmark = pytest.mark.gpu

HB_EINVAL = -1
_PRIMES = load_golden("mixed_primes.json")
_SEEDS = {20: 2020, 61: 2061, 129: 2129, 256: 2256, 257: 2257, 512: 2512, 1000: 3000, 1024: 3024, 1025: 3025, 2048: 4048}


def recorded_prime(bits):
    """The prime of `bits` bits that tests/golden/mixed_primes.json records."""
    return int(_PRIMES["%d/%d" % (bits, _SEEDS[bits])], 16)


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


def geometry(p, S):
    ss = p.bit_length() // 8
    return ss, ss * S


def nblocks(p, S, n):
    return n // geometry(p, S)[1] + 1


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def mfile(rng, p, S, length, klen=32):
    """(p, S, f_key, alpha_key, file bytes), seeded."""
    return (p, S, _bytes(rng, klen), _bytes(rng, klen), _bytes(rng, length))


def encode_mixed(nat, items, cxx=False, flags=0, data_ptrs=None, tag_ptrs=None, edit=None, fill=0xA5):
    """hb_encode_mixed (cxx: hb_cxx_encode_mixed) over items (p, S, f_key,
    alpha_key, file bytes): (rc, [tag bytes per file] for host tags, tries,
    launches).  Host buffers unless data_ptrs / tag_ptrs give device addresses;
    edit(descs) may spoil descriptors before the call."""
    ctx = nat.context()
    n = len(items)
    descs = (nat.EncodeMixedDesc * max(n, 1))()
    keep, outs = [], []
    for i, (p, S, fk, ak, data) in enumerate(items):
        pb = nat.be(p)
        a = np.frombuffer(data, dtype=np.uint8)
        good = p.bit_length() >= 8 and S >= 1
        out = np.full((nblocks(p, S, len(data)) if good else 4) * max(nat.width_of(p), 1), fill, dtype=np.uint8)
        keep.append((pb, a))
        outs.append(out)
        d = descs[i]
        d.p_be, d.p_len, d.sectors, d.key_len = pb, len(pb), S, len(fk)
        d.f_key, d.alpha_key = fk, ak
        d.data = data_ptrs[i] if data_ptrs is not None else (a.ctypes.data if len(a) else None)
        d.len = len(data)
        d.tags = tag_ptrs[i] if tag_ptrs is not None else out.ctypes.data
    if edit:
        edit(descs)
    tries = ctypes.c_uint64(12345)
    with ctx.lock:
        rc = getattr(nat.lib(), "hb_cxx_encode_mixed" if cxx else "hb_encode_mixed")(ctx.h, descs, n, flags, ctypes.byref(tries))
    launches = ctx.last_kernel_ms()[1] if rc == 0 else None
    return rc, [o.tobytes() for o in outs], tries.value, launches


def encode_single(nat, item, cxx=False):
    """One host-buffer hb_encode of a whole file (cxx: with HB_PRF_CXX): (tag bytes, tries)."""
    p, S, fk, ak, data = item
    ctx = nat.context()
    nb = nblocks(p, S, len(data))
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(nb * nat.width_of(p), dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), 0, a.ctypes.data if len(a) else None,
                                      len(data), nb, out.ctypes.data, nat.HB_PRF_CXX if cxx else 0, ctypes.byref(tries)))
    return out.tobytes(), tries.value


def oracle_raw(oracle, item, cxx=False):
    p, S, fk, ak, data = item
    w = (p.bit_length() + 7) // 8
    return b"".join(t.to_bytes(w, "big") for t in (oracle.cxx_encode if cxx else oracle.encode)(p, S, fk, ak, data))


def what(item):
    return (item[0].bit_length(), item[1], len(item[2]), len(item[4]))


def check_mixed(nat, oracle, items, cxx=False, single=True, **kw):
    """The mixed call == hb_encode per file == the oracle's encode, every
    file; tries == the sum of the single calls' tries."""
    rc, got, tries, launches = encode_mixed(nat, items, cxx=cxx, **kw)
    assert rc == 0, last_error(nat)
    total = 0
    for i, it in enumerate(items):
        if single:
            one, t = encode_single(nat, it, cxx)
            total += t
            assert got[i] == one, (i,) + what(it)
        assert got[i] == oracle_raw(oracle, it, cxx), (i,) + what(it)
    if single:
        assert tries == total
    return got, tries, launches


def boundary_lengths(p, S, T=256):
    """The lengths at which a file's own geometry changes the work: 0, 1, the
    sector and block boundaries, a short last block, and T / S and T / S + 1
    blocks where the file crosses a MAC workgroup."""
    ss, C = geometry(p, S)
    bpw = T // S if 2 <= S <= T else 256
    return sorted({0, 1, max(ss - 1, 0), ss, ss + 1, C - 1, C, C + 1, 3 * C + 17, bpw * C - 1, bpw * C + 1})


def untouched(got):
    return all(set(g) <= {0xA5} for g in got)


# ------------------------------------------------------------------ 1: one prime, one S
def test_one_prime_equals_encode_many(nat, oracle):
    from test_gpu_encode_many import encode_many
    S = 10
    rng = np.random.default_rng(10)
    items = [mfile(rng, P256, S, ln) for ln in boundary_lengths(P256, S) + [5000, 12345]]
    got, tries, launches = check_mixed(nat, oracle, items)
    assert launches == 3                                          # PRF, conversion, one MAC shape
    rc, many, tries1 = encode_many(nat, P256, S, [it[2:4] for it in items], [it[4] for it in items])
    assert rc == 0 and many == got and tries1 == tries


# ------------------------------------------------------------------ 2: neighbours that differ
_neigh = {}


def neighbours(nat, oracle):
    """36 files, one limb class, every neighbour under another modulus,
    geometry (ss 16 / 31 / 32) and S; checked once against hb_encode and the oracle."""
    if not _neigh:
        rng = np.random.default_rng(20)
        primes, sectors = [recorded_prime(129), P255, P256], [2, 3, 10]
        items = []
        for i in range(36):
            p, S = primes[i % 3], sectors[(i + i // 3) % 3]
            ss, C = geometry(p, S)
            items.append(mfile(rng, p, S, [0, C - 1, 3 * C + 17, 40 * C + 1, ss + 1, C][i % 6]))
        assert len({(it[0], it[1]) for it in items}) == 9
        for a, b in zip(items, items[1:]):
            assert a[0] != b[0] and a[1] != b[1]
        got, tries, launches = check_mixed(nat, oracle, items)
        _neigh["v"] = (items, got, tries, launches)
    return _neigh["v"]


def test_neighbours_that_differ_in_three_orders(nat, oracle):
    items, got, tries, launches = neighbours(nat, oracle)
    assert launches == 3                                          # one class, one group, one MAC shape
    order = [k for pair in zip(range(18), range(35, 17, -1)) for k in pair]   # interleaved from both ends
    for perm in (list(reversed(range(36))), order):
        rc, again, tries2, launches = encode_mixed(nat, [items[k] for k in perm])
        assert rc == 0 and launches == 3
        assert again == [got[k] for k in perm]
        assert tries2 == tries


# ------------------------------------------------------------------ 3: S at every MAC boundary
@pytest.mark.parametrize("bits,T", [(256, 256), (1024, 256), (2048, 128)])
def test_sector_counts_at_every_mac_boundary(nat, oracle, bits, T):
    """1, 2, 3, 16, 17: the alpha wave-job boundary; T - 1, T, T + 1: the split
    shape against the lane-per-block shape; 255, 256, 257: the conversion
    pass's workgroup boundary -- as neighbours in one group."""
    p = P256 if bits == 256 else recorded_prime(bits)
    rng = np.random.default_rng(30 + bits)
    items = []
    for S in sorted({1, 2, 3, 16, 17, T - 1, T, T + 1, 255, 256, 257}):
        ss, C = geometry(p, S)
        # one block; two; one MAC workgroup and a block (S > T: 256 blocks of
        # T + 1 sectors would be megabytes -- S = 1 crosses the lane shape's)
        for ln in (0, C + ss + 1, (T // S if 2 <= S <= T else 256) * C + 1 if S <= T else 2 * C + 5):
            items.append(mfile(rng, p, S, ln))
    got, tries, launches = check_mixed(nat, oracle, items)
    assert launches == 4                                          # both MAC shapes in the one group


# ------------------------------------------------------------------ 4: file lengths per geometry
def test_file_lengths_at_each_files_own_boundaries(nat, oracle):
    rng = np.random.default_rng(40)
    shapes = [(P256, 10), (P255, 3), (recorded_prime(129), 16), (P256MAX, 1), (recorded_prime(20), 3), (recorded_prime(61), 10)]
    per = [[mfile(rng, p, S, ln) for ln in boundary_lengths(p, S)] for p, S in shapes]
    # interleaved: a file's neighbours have other geometries
    items = [per[k][i] for i in range(max(len(x) for x in per)) for k in range(len(per)) if i < len(per[k])]
    got, tries, launches = check_mixed(nat, oracle, items)
    assert launches == 4
    # a 1024-bit and a 2048-bit file crossing a MAC workgroup (T = 256 and 128)
    items = []
    for bits, S, T in ((1024, 10, 256), (2048, 4, 128), (1000, 7, 256), (1025, 3, 128)):
        p = recorded_prime(bits)
        items += [mfile(rng, p, S, ln) for ln in boundary_lengths(p, S, T)]
    check_mixed(nat, oracle, items)


# ------------------------------------------------------------------ 5: every class and key size in one call
def test_every_class_and_key_size_in_one_call(nat, oracle):
    S = 3
    items = []
    for bits in (20, 61, 129, 256, 257, 512, 1000, 1024, 1025, 2048):
        p = recorded_prime(bits)
        ss, C = geometry(p, S)
        for klen in (16, 24, 32):
            rng = np.random.default_rng(bits + klen)
            items += [mfile(rng, p, S, ln, klen=klen) for ln in (0, 4 * C + ss // 2 + 1, C - 1)]
    assert len(items) == 90
    got, tries, launches = check_mixed(nat, oracle, items)
    assert launches == 36                                         # 4 limb classes x 3 round counts, 3 launches each


# ------------------------------------------------------------------ 6: the reference's recorded encodes
def test_golden_encodes_in_one_call(nat, golden_encode):
    items, wants, names = [], [], []
    for c in golden_encode["cases"]:
        p = int(c["prime"], 16)
        w = nat.width_of(p)
        wants.append(b"".join(int(t, 16).to_bytes(w, "big") for t in c["tags"]))
        items.append((p, c["sectors"], bytes.fromhex(c["f_key"]), bytes.fromhex(c["alpha_key"]), bytes.fromhex(c["data"])))
        names.append(c["name"])
    assert len(items) == 176
    # what the file records: primes of 20 to 1024 bits (two limb classes), four sector counts
    assert {it[0].bit_length() for it in items} == {20, 61, 255, 256, 1024} and {it[1] for it in items} == {1, 3, 10, 16}
    rc, got, tries, launches = encode_mixed(nat, items)
    assert rc == 0, last_error(nat)
    for g, want, name in zip(got, wants, names):
        assert g == want, name
    assert tries >= sum(len(g) // nat.width_of(it[0]) for g, it in zip(got, items))


# ------------------------------------------------------------------ 7: equal inputs, repeated primes
def test_equal_bytes_and_keys_under_different_primes(nat, oracle):
    rng = np.random.default_rng(70)
    fk, ak, data = _bytes(rng, 32), _bytes(rng, 32), _bytes(rng, 1500)
    primes = [P256, P255, recorded_prime(129), P256MAX, P256, recorded_prime(61), P255, P256]
    items = [(p, 4, fk, ak, data) for p in primes]
    got, tries, launches = check_mixed(nat, oracle, items)
    assert got[0] == got[4] == got[7] and got[1] == got[6]       # the same prime on non-adjacent files
    assert len(set(got)) == 5                                     # and nothing else coincides


# ------------------------------------------------------------------ 8: where the bytes live
def device_case(nat, oracle, items, want, cxx=False):
    """Device-resident data and tags at odd addresses with differing 16-byte
    alignment between neighbours; host data with device tags; the reverse."""
    doffs, toffs, d, t = [], [], 1, 3
    for k, it in enumerate(items):
        doffs.append(d)
        toffs.append(t)
        d = d + len(it[4]) + 1 + 2 * (k % 7)
        t = t + len(want[k]) + 1 + 2 * (k % 5)
    assert len({o % 16 for o in doffs}) > 2 and len({o % 16 for o in toffs}) > 2
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    try:
        for it, o in zip(items, doffs):
            dbuf.upload(it[4], o)
        dp, tp = [dbuf.p + o for o in doffs], [tbuf.p + o for o in toffs]
        for flags, kw in ((3, dict(data_ptrs=dp, tag_ptrs=tp)), (2, dict(tag_ptrs=tp)), (1, dict(data_ptrs=dp))):
            if flags & 2:
                tbuf.upload(b"\xa5" * tbuf.n)
            rc, got, tries, launches = encode_mixed(nat, items, cxx=cxx, flags=flags, **kw)
            assert rc == 0, last_error(nat)
            if flags & 2:
                raw = tbuf.download()
                for k in range(len(items)):
                    assert raw[toffs[k]:toffs[k] + len(want[k])] == want[k], (flags, k) + what(items[k])
                    assert raw[toffs[k] + len(want[k])] == 0xA5, (flags, k)     # nothing past the file's tags
                assert untouched(got)                                          # the host buffers were not the target
            else:
                assert got == want, flags
    finally:
        dbuf.free()
        tbuf.free()


def test_device_and_host_resident_mixes(nat, oracle):
    items, got, tries, launches = neighbours(nat, oracle)
    rng = np.random.default_rng(80)
    p1024 = recorded_prime(1024)
    wide = [mfile(rng, p1024, 10, ln) for ln in (0, 1279, 1280 * 3, 5000)]      # 16-byte sectors possible: C = 1280
    wgot, _, _ = check_mixed(nat, oracle, wide)
    device_case(nat, oracle, items[:20] + wide, got[:20] + wgot)


# ------------------------------------------------------------------ 9: splitting, fall-through
def test_group_splitting(nat, oracle, monkeypatch):
    items, want, tries, _ = neighbours(nat, oracle)
    blocks = [nblocks(it[0], it[1], len(it[4])) for it in items]
    cap = max(sum(blocks) // 3, max(blocks))
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", str(cap))
    try:
        rc, got, tries2, launches = encode_mixed(nat, items)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want and tries2 == tries
    assert launches >= 9                                          # at least three groups of three launches


def large_file_case(nat, oracle, monkeypatch, cxx):
    rng = np.random.default_rng(90)
    p512 = recorded_prime(512)
    items = [mfile(rng, P256, 16, 5 * 512 + 3), mfile(rng, p512, 5, 40 * 320 + 9), mfile(rng, P255, 3, 700),
             mfile(rng, p512, 5, 2 * 320)]
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", "12")              # the second file has 41 blocks
    try:
        got, tries, launches = check_mixed(nat, oracle, items, cxx=cxx)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert launches > 6                                           # two classes' groups and a single encode


def test_large_file_falls_through_under_its_own_prime(nat, oracle, monkeypatch):
    large_file_case(nat, oracle, monkeypatch, False)


# ------------------------------------------------------------------ 10: rejected descriptors
def rejected_cases(nat, cxx=False):
    def null(field):
        def f(d):
            setattr(d, field, None)
        return f

    def set_to(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    even, tiny = nat.be(P256 - 1), nat.be(127)
    huge = nat.be((1 << 2048) | 1)
    cases = [("an even prime", set_to(p_be=even, p_len=len(even)), HB_EINVAL),
             ("a prime below 2^8", set_to(p_be=tiny, p_len=len(tiny)), HB_EINVAL),
             ("a prime above 2048 bits", set_to(p_be=huge, p_len=len(huge)), nat.HB_EUNSUPPORTED),
             ("an empty prime", set_to(p_len=0), HB_EINVAL),
             ("sectors == 0", set_to(sectors=0), HB_EINVAL),
             ("sectors == 2^32", set_to(sectors=1 << 32), HB_EINVAL),
             ("a bad key length", set_to(key_len=20), HB_EINVAL),
             ("a NULL f_key", null("f_key"), HB_EINVAL),
             ("a NULL alpha_key", null("alpha_key"), HB_EINVAL),
             ("a NULL tag buffer", null("tags"), HB_EINVAL),
             ("a NULL data buffer with len > 0", null("data"), HB_EINVAL)]
    if cxx:
        odd = nat.be(recorded_prime(1000))
        cases.append(("a ByteCount that is no multiple of 16", set_to(p_be=odd, p_len=len(odd)), nat.HB_EUNSUPPORTED))
    return cases, (even, tiny, huge)


def check_rejected(nat, items, cxx=False):
    cases, keep = rejected_cases(nat, cxx)
    for name, spoil, code in cases:
        for at in (0, 3, len(items) - 1):
            if name == "a NULL data buffer with len > 0" and not items[at][4]:
                continue                                          # (an empty file may have no buffer)
            rc, got, tries, _ = encode_mixed(nat, items, cxx=cxx, edit=lambda descs: spoil(descs[at]))
            assert rc == code, (name, at, rc, last_error(nat))
            assert last_error(nat).startswith("file %d: " % at), (name, last_error(nat))
            assert untouched(got), (name, at)
            assert tries == 0


def test_each_rejected_descriptor(nat, oracle):
    items, _, _, _ = neighbours(nat, oracle)
    check_rejected(nat, items[:6])


# ------------------------------------------------------------------ 11: flags, the empty call
@pytest.mark.parametrize("flag", ["HB_PRF_CXX", "HB_ASYNC", "HB_ENCODE_SINGLE_PASS"])
def test_unsupported_flags(nat, oracle, flag):
    items, _, _, _ = neighbours(nat, oracle)
    rc, got, _, _ = encode_mixed(nat, items[:4], flags=getattr(nat, flag))
    assert rc == nat.HB_EUNSUPPORTED
    assert untouched(got)


def test_empty_call(nat):
    rc, got, tries, _ = encode_mixed(nat, [])
    assert rc == 0 and got == [] and tries == 0
    ctx = nat.context()
    with ctx.lock:
        assert nat.lib().hb_encode_mixed(ctx.h, None, 0, 0, None) == 0
        assert nat.lib().hb_encode_mixed(ctx.h, None, 2, 0, None) == HB_EINVAL


# ------------------------------------------------------------------ 12: the context afterwards
def test_context_left_clean(nat, oracle, pys):
    from test_gpu_encode_many import encode_many
    items, got, _, _ = neighbours(nat, oracle)
    rc, again, _, _ = encode_mixed(nat, items[:9])
    assert rc == 0 and again == got[:9]
    # hb_encode_many, a prove, a verify and a plain encode all equal the oracle
    rng = np.random.default_rng(120)
    S = 10
    many = [mfile(rng, P256, S, ln) for ln in (0, 319, 320, 2000)]
    rc, tags, _ = encode_many(nat, P256, S, [it[2:4] for it in many], [it[4] for it in many])
    assert rc == 0 and tags == [oracle_raw(oracle, it) for it in many]
    it = many[3]
    proof_item = (_bytes(rng, 32), 9, P256, tags[3], it[4])
    rc, proof = prove_single(nat, P256, S, proof_item)
    assert rc == 0 and proof == oracle_proof(oracle, P256, S, proof_item)
    beat = pys.PySwizzle(S, b"k" * 32, P256)
    state = pys.State(it[2], it[3], len(tags[3]) // 32)
    state.encrypt(beat.key)
    pr = pys.Proof()
    pr.mu = [int.from_bytes(proof[0][j * 32:(j + 1) * 32], "big") for j in range(S)]
    pr.sigma = int.from_bytes(proof[1], "big")
    assert beat.verify(pr, pys.Challenge(9, P256, proof_item[0]), state)
    assert encode_single(nat, it)[0] == oracle_raw(oracle, it)


# ------------------------------------------------------------------ 13: end to end
def end_to_end(beats, mod, rng):
    """encode_mixed -> prove_mixed -> verify_mixed over three beats; one file
    tampered after the encode fails for that item alone."""
    cls = type(beats[0])
    blobs = [_bytes(rng, n) for n in (0, 700, 5000, 1, 3333, 12000, 64, 2049, 900)]
    items = [(beats[k % 3], io.BytesIO(b)) for k, b in enumerate(blobs)]
    res = cls.encode_mixed(items)
    assert len(res) == 9 and all(f.tell() == len(b) for (_, f), b in zip(items, blobs))
    chals = [beat.gen_challenge(state) for (beat, _), (tag, state) in zip(items, res)]
    stored = list(blobs)
    bad = bytearray(stored[5])
    bad[len(bad) // 2] ^= 1
    stored[5] = bytes(bad)
    # 64 draws per block: the flipped byte's block is missed by all of them with probability < e^-64
    chals[5] = mod.Challenge(64 * len(res[5][0]), beats[5 % 3].prime, b"\x21" * 32)
    proofs = cls.prove_mixed([(beat.get_public(), io.BytesIO(b), c, tag)
                              for (beat, _), b, c, (tag, _) in zip(items, stored, chals, res)])
    ok = cls.verify_mixed([(beat, pr, c, state) for (beat, _), pr, c, (_, state) in zip(items, proofs, chals, res)])
    assert ok == [k != 5 for k in range(9)]
    return res


def test_encode_prove_verify_mixed_end_to_end(nat, oracle, pys):
    beats = [pys.PySwizzle(16, b"a" * 32, P256), pys.PySwizzle(10, b"b" * 32, recorded_prime(1024)),
             pys.PySwizzle(3, b"c" * 32, recorded_prime(61))]
    res = end_to_end(beats, pys, np.random.default_rng(130))
    # the loop's results under the same keys
    tag, state = res[4]
    state.decrypt(beats[1].key)
    blob = _bytes(np.random.default_rng(131), 10)
    assert pys.encode_file(int(beats[1].prime), 10, state.f_key, state.alpha_key, io.BytesIO(blob))[0].sigma == \
        oracle.encode(beats[1].prime, 10, state.f_key, state.alpha_key, blob)
