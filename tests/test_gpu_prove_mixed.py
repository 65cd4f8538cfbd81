"""GPU parity of the mixed-owner batched prove (hb_prove_mixed,
PySwizzle.prove_mixed): mu and sigma of many proofs that each name their own
prime, sector count and key length, in three launches per group of a (limb
count, AES round count) class (hb_mixed.hpp; hb_runtime.cpp prove_mixed_impl).

Every comparison is byte for byte, every item of every batch: the mixed call
against hb_prove per proof and against the CPU oracle's prove.  Over

* one prime (== hb_prove_many), neighbours that differ in modulus, geometry and
  column count inside one group, in three orders,
* every limb class and key size in one call, the reference's recorded proofs
  (tests/golden/encode_cases.json) in one call,
* factors that are not below p next to ones that are, a v_max that is too wide
  for one proof's prime and fits another's,
* the conversion pass's workgroup boundaries, device- and host-resident data
  with differing 16-byte alignment between neighbours,
* group splitting and the fall-throughs under each proof's own prime, errors,
* PySwizzle.prove_mixed / verify_mixed end to end.

Reference: a storage node's loop over PySwizzle.py:333-370 for many owners
(one prime per PySwizzle instance, :250-251)."""
import ctypes
import importlib
import io
import random

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import P256, DevBuf
from test_gpu_primes import seeded_prime
from test_gpu_prove_many import P255, P256MAX, _bytes, _item, last_error, oracle_proof, prove_many, prove_single
from heartbeat_amd.exc import HeartbeatError

pytestmark = pytest.mark.gpu

HB_EINVAL = -1
_PRIMES = load_golden("mixed_primes.json")


def recorded_prime(bits, seed):
    """seeded_prime(bits, seed) as tests/golden/mixed_primes.json records it
    (the search for a 2048-bit prime alone takes seconds)."""
    return int(_PRIMES["%d/%d" % (bits, seed)], 16)


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


def mitem(rng, p, S, chunks, length, ntags=None, vmax=None, klen=32):
    """(p, S) + test_gpu_prove_many's item (chal_key, chunks, v_max, tag bytes, file bytes)."""
    return (p, S) + _item(rng, p, S, chunks, length, ntags=ntags, vmax=vmax, klen=klen)


def fill_descs(nat, items, out, offs, data_ptrs=None, tag_ptrs=None):
    descs = (nat.ProveMixedDesc * max(len(items), 1))()
    keep = []
    for i, (p, S, ck, chunks, vmax, tags, data) in enumerate(items):
        w = nat.width_of(p)
        pb, vb = nat.be(p), nat.be(vmax)
        t, a = np.frombuffer(tags, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
        keep.append((pb, vb, t, a))
        d = descs[i]
        d.p_be, d.p_len, d.sectors, d.key_len = pb, len(pb), S, len(ck)
        d.chal_key, d.chunks = ck, chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.tags = tag_ptrs[i] if tag_ptrs is not None else (t.ctypes.data if len(t) else None)
        d.ntags = len(tags) // w
        d.data = data_ptrs[i] if data_ptrs is not None else (a.ctypes.data if len(a) else None)
        d.len = len(data)
        d.mu_out = out.ctypes.data + offs[i]
        d.sigma_out = out.ctypes.data + offs[i] + S * w
    return descs, keep


def prove_mixed(nat, items, flags=0, data_ptrs=None, tag_ptrs=None, edit=None, fill=0xA5):
    """hb_prove_mixed over items (p, S, chal_key, chunks, v_max, tag bytes,
    file bytes): (rc, [(mu bytes, sigma bytes) per proof], launches).  edit(descs)
    may spoil descriptors before the call."""
    ctx = nat.context()
    offs, total = [], 0
    for it in items:
        offs.append(total)
        total += (it[1] + 1) * nat.width_of(it[0]) if it[0] else 0
    out = np.full(max(total, 1), fill, dtype=np.uint8)
    descs, keep = fill_descs(nat, items, out, offs, data_ptrs, tag_ptrs)
    if edit:
        edit(descs)
    with ctx.lock:
        rc = nat.lib().hb_prove_mixed(ctx.h, descs, len(items), flags)
    launches = ctx.last_kernel_ms()[1] if rc == 0 else None
    raw = out.tobytes()
    res = []
    for it, o in zip(items, offs):
        w = nat.width_of(it[0]) if it[0] else 0
        res.append((raw[o:o + it[1] * w], raw[o + it[1] * w:o + (it[1] + 1) * w]))
    return rc, res, launches


def untouched(out):
    return all(set(m) | set(s) <= {0xA5} for m, s in out)


def check_mixed(nat, oracle, items, single=True, **kw):
    """The mixed call == hb_prove per proof == the oracle's prove, every item."""
    rc, got, launches = prove_mixed(nat, items, **kw)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        p, S = it[:2]
        if single:
            rc1, one = prove_single(nat, p, S, it[2:])
            assert rc1 == 0, last_error(nat)
            assert got[i] == one, (i, p.bit_length(), S, it[3], len(it[6]))
        assert got[i] == oracle_proof(oracle, p, S, it[2:]), (i, p.bit_length(), S, it[3], len(it[6]))
    return got, launches


def test_recorded_primes_are_the_seeded_ones():
    for bits in (20, 61, 129, 256, 257):
        assert recorded_prime(bits, 2000 + bits) == seeded_prime(bits, 2000 + bits)
    for key, hexp in _PRIMES.items():
        if "/" in key:
            assert int(hexp, 16).bit_length() == int(key.split("/")[0]) and int(hexp, 16) % 2 == 1


# ------------------------------------------------------------------ 4: one prime
def test_one_prime_equals_prove_many(nat, oracle):
    S = 10
    C = 32 * S
    rng = np.random.default_rng(40)
    items = [mitem(rng, P256, S, n, ln) for n in (0, 1, 16, 17, 33, 257) for ln in (0, 1, C - 1, C + 1, 3 * C + 17)]
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 3
    rc, many = prove_many(nat, P256, S, [it[2:] for it in items])
    assert rc == 0 and many == got
    w = nat.width_of(P256)
    for it, (mu, sg) in zip(items, got):
        if it[3] == 0:
            assert mu == bytes(S * w) and sg == bytes(w)


# ------------------------------------------------------------------ 5: neighbours that differ
_neigh = {}


def neighbours(nat, oracle):
    """36 proofs, one limb class, every neighbour under another modulus,
    geometry and column count; checked once against hb_prove and the oracle."""
    if not _neigh:
        rng = np.random.default_rng(50)
        primes, sectors, chunks = [P256, P256MAX, P255], [1, 3, 10], [1, 15, 16, 17, 33, 257]
        items = []
        for i in range(36):
            p, S, n = primes[i % 3], sectors[(i + i // 3) % 3], chunks[(i + i // 6) % 6]
            C = (p.bit_length() // 8) * S
            items.append(mitem(rng, p, S, n, [0, C - 1, 3 * C + 17, 40 * C + 1][i % 4]))
        assert len({(it[0], it[1]) for it in items}) == 9 and {it[3] for it in items} == set(chunks)
        for a, b in zip(items, items[1:]):
            assert a[0] != b[0] and a[1] != b[1]
        got, launches = check_mixed(nat, oracle, items)
        _neigh["v"] = (items, got, launches)
    return _neigh["v"]


def test_neighbours_that_differ(nat, oracle):
    items, got, launches = neighbours(nat, oracle)
    assert launches == 3                                          # one class, one group
    order = list(range(36))
    random.Random(51).shuffle(order)
    for perm in (list(reversed(range(36))), order):
        rc, again, launches = prove_mixed(nat, [items[k] for k in perm])
        assert rc == 0 and launches == 3
        assert again == [got[k] for k in perm]


# ------------------------------------------------------------------ 6: every class and key size in one call
def test_every_class_and_key_size_in_one_call(nat, oracle):
    S = 3
    items = []
    for bits in (20, 61, 129, 256, 257, 512, 1000, 1024, 1025, 2048):
        p = recorded_prime(bits, 2000 + bits)
        C = (bits // 8) * S
        for klen in (16, 24, 32):
            rng = np.random.default_rng(bits + klen)
            items += [mitem(rng, p, S, n, ln, klen=klen) for n, ln in [(1, 0), (17, 4 * C + (bits // 8) // 2 + 1), (33, C - 1)]]
    assert len(items) == 90
    got, launches = check_mixed(nat, oracle, items, single=False)
    assert launches == 36                                         # 4 limb classes x 3 round counts, 3 launches each


# ------------------------------------------------------------------ 7: the reference's recorded proofs
def test_golden_proofs_in_one_call(nat, golden_encode):
    items, wants, names = [], [], []
    for c in golden_encode["cases"]:
        p = int(c["prime"], 16)
        w = nat.width_of(p)
        tags = b"".join(int(t, 16).to_bytes(w, "big") for t in c["tags"])
        data = bytes.fromhex(c["data"])
        for chn, prn in (("chal", "proof"), ("chal2", "proof2")):
            ch = c[chn]
            wants.append((b"".join(int(m, 16).to_bytes(w, "big") for m in c[prn]["mu"]),
                          int(c[prn]["sigma"], 16).to_bytes(w, "big")))
            items.append((p, c["sectors"], bytes.fromhex(ch["key"]), ch["chunks"], int(ch["v_max"], 16), tags, data))
            names.append(c["name"])
    assert len(items) == 352
    # what the file records: six primes (20 to 1024 bits: two limb classes),
    # four sector counts, 32-byte challenge keys -- one call, where the
    # one-prime batch needs one per (prime, S)
    assert len({it[0] for it in items}) == 6 and {it[1] for it in items} == {1, 3, 10, 16}
    assert {len(it[2]) for it in items} == {32}
    rc, got, _ = prove_mixed(nat, items)
    assert rc == 0, last_error(nat)
    for g, want, name in zip(got, wants, names):
        assert g == want, name


# ------------------------------------------------------------------ 8: factors not below p
def test_factors_not_below_p_next_to_ones_that_are(nat, oracle):
    S = 3
    rng = np.random.default_rng(80)
    big = [(P256MAX, S, _bytes(rng, 32), n, (1 << 256) - 1, b"\xff" * (32 * nt), b"\xff" * ln)
           for n, ln, nt in [(1, 96, 2), (17, 96 * 5 + 31, 6), (300, 96 * 9, 10)]]
    small = [mitem(rng, P255, S, n, 1000, vmax=2) for n in (1, 37, 300)]
    items = [x for pair in zip(big, small) for x in pair]
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 3
    # a v_max of 257 bits: too wide for a 256-bit prime's limbs, inside a 512-bit prime's
    p512 = recorded_prime(512, 2512)
    wide = (1 << 256) + 1
    ok512 = mitem(rng, p512, S, 5, 1000, vmax=wide)
    bad256 = mitem(rng, P255, S, 5, 1000, vmax=wide)
    assert prove_single(nat, P255, S, bad256[2:])[0] == nat.HB_EUNSUPPORTED
    rc, out, _ = prove_mixed(nat, items[:3] + [ok512, bad256] + items[3:])
    assert rc == nat.HB_EUNSUPPORTED and "proof 4" in last_error(nat)
    assert untouched(out)                                         # before any work
    got2, _ = check_mixed(nat, oracle, items[:3] + [ok512] + items[3:])
    assert got2[:3] + got2[4:] == got


# ------------------------------------------------------------------ 9: conversion-pass boundaries
def test_conversion_pass_boundaries(nat, oracle):
    """A proof's terms end inside, at and one past a 256-thread workgroup of
    the conversion pass, under alternating primes."""
    rng = np.random.default_rng(90)
    items = []
    for i, n in enumerate((255, 256, 257, 1, 511, 512, 513)):
        p, S = (P256MAX, 2) if i % 2 else (P255, 3)
        items.append(mitem(rng, p, S, n, 40 * (p.bit_length() // 8) * S + 5))
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 3


# ------------------------------------------------------------------ 10: residency
@pytest.fixture(scope="module")
def resident(nat, oracle):
    """16 proofs of mixed primes and S, their host-buffer call checked once, and
    the files and tags on the device: odd byte offsets for the odd proofs,
    16-byte-aligned ones for the even proofs, so that HB_PB_LOAD16 differs
    between neighbours (P256 / P256MAX proofs with full-width sectors)."""
    rng = np.random.default_rng(100)
    shapes = [(1, 0, 1), (16, 1, 2), (17, 3, 7), (33, 60, None), (257, 200, None), (40, 1, 1), (5, 0, 1), (100, 0, 3)] * 2
    combos = [(P256, 10), (P256MAX, 2), (P256, 4), (P255, 3)]
    items = []
    for i, (n, blocks, nt) in enumerate(shapes):
        p, S = combos[i % 4]
        C = (p.bit_length() // 8) * S
        items.append(mitem(rng, p, S, n, blocks * C + (17 if i % 3 else 0), nt))
    want, launches = check_mixed(nat, oracle, items)
    assert launches == 3
    doffs, toffs, d, t = [], [], 0, 0
    for i, it in enumerate(items):
        d, t = (d + 15) & ~15, (t + 15) & ~15
        if i % 2:
            d, t = d + 1, t + 3
        doffs.append(d)
        toffs.append(t)
        d += len(it[6])
        t += len(it[5])
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    assert dbuf.p % 16 == 0 and tbuf.p % 16 == 0
    for it, do, to in zip(items, doffs, toffs):
        dbuf.upload(it[6], do)
        tbuf.upload(it[5], to)
    yield items, want, [dbuf.p + o for o in doffs], [tbuf.p + o for o in toffs]
    dbuf.free()
    tbuf.free()


@pytest.mark.parametrize("flags", [3, 1, 2])
def test_residency(nat, resident, flags):
    items, want, dptrs, tptrs = resident
    rc, got, launches = prove_mixed(nat, items, flags=flags, data_ptrs=dptrs if flags & 1 else None,
                                    tag_ptrs=tptrs if flags & 2 else None)
    assert rc == 0, last_error(nat)
    assert got == want
    if flags != 2:                                                # (2: host data with device tags, the single prove)
        assert launches == 3


# ------------------------------------------------------------------ 11: splitting, fall-through
def test_group_splitting_and_long_challenges(nat, oracle, monkeypatch):
    items, want, _ = neighbours(nat, oracle)
    rng = np.random.default_rng(110)
    p1024 = recorded_prime(1024, 3024)
    longs = [mitem(rng, P255, 3, 1000, 5000), mitem(rng, p1024, 2, 1000, 9000)]
    lwant, _ = check_mixed(nat, oracle, longs)
    batch = items[:20] + [longs[0]] + items[20:] + [longs[1]]
    total = sum(it[3] for it in items)
    assert total > 4 * 300
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "300")
    try:
        rc, got, launches = prove_mixed(nat, batch)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want[:20] + [lwant[0]] + want[20:] + [lwant[1]]  # the bytes do not change
    assert launches >= 3 * 5 + 2                                  # several groups, and the two single proves
    rc, got, launches = prove_mixed(nat, batch)
    assert rc == 0 and launches == 6 and got == want[:20] + [lwant[0]] + want[20:] + [lwant[1]]


def test_host_file_not_uploaded_falls_through(nat, oracle):
    rng = np.random.default_rng(111)
    p1024 = recorded_prime(1024, 3024)
    small = [mitem(rng, P256, 2, n, ln) for n, ln in ((17, 5000), (3, 64))]
    items = [small[0], mitem(rng, p1024, 2, 5, (8 << 20) + 1), small[1]]
    got, launches = check_mixed(nat, oracle, items)
    assert 3 < launches <= 5                                      # one group of the small ones, then the single prove
    rc, alone, launches = prove_mixed(nat, small)
    assert rc == 0 and launches == 3 and alone == [got[0], got[2]]


# ------------------------------------------------------------------ 12: errors, no-ops
def test_errors_and_noops(nat, oracle):
    rng = np.random.default_rng(120)
    items = [mitem(rng, P256, 4, 3, 700), mitem(rng, P255, 2, 20, 700), mitem(rng, P256MAX, 3, 0, 700)]
    want, _ = check_mixed(nat, oracle, items)

    def valid():
        rc, got, _ = prove_mixed(nat, items)
        assert rc == 0 and got == want

    rc, got, _ = prove_mixed(nat, [])
    assert rc == 0 and got == []
    for flags in (nat.HB_PRF_CXX, nat.HB_ASYNC | 3, nat.HB_ENCODE_SINGLE_PASS, 1 << 20):
        rc, got, _ = prove_mixed(nat, items, flags=flags)
        assert rc == nat.HB_EUNSUPPORTED and untouched(got)
    valid()
    # what hb_prove rejects for the proof's own arguments, at item 1 of 3, with its code
    p2049 = (1 << 2048) | 1
    pb2049, pb7 = nat.be(p2049), nat.be(0x7f)

    def spoil(**fields):
        def edit(descs):
            for k, v in fields.items():
                setattr(descs[1], k, v)
        return edit

    it1 = items[1]
    cases = [(spoil(p_be=pb2049, p_len=len(pb2049)), prove_single(nat, p2049, 2, it1[2:])[0]),
             (spoil(p_be=pb7, p_len=1), prove_single(nat, 0x7f, 2, it1[2:])[0]),
             (spoil(p_len=0), HB_EINVAL),
             (spoil(p_be=None), HB_EINVAL),
             (spoil(sectors=0), prove_single(nat, P255, 0, it1[2:])[0]),
             (spoil(key_len=15), HB_EINVAL),
             (spoil(ntags=0), HB_EINVAL),
             (spoil(vmax_len=0), HB_EINVAL)]                       # v_max == 0
    cases += [(spoil(**{f: None}), HB_EINVAL) for f in ("chal_key", "vmax_be", "tags", "data", "mu_out", "sigma_out")]
    assert cases[0][1] == nat.HB_EUNSUPPORTED and cases[1][1] == HB_EINVAL and cases[4][1] == HB_EINVAL
    for edit, code in cases:
        rc, got, _ = prove_mixed(nat, items, edit=edit)
        assert rc == code and "proof 1" in last_error(nat), last_error(nat)
        assert untouched(got)
    valid()
    ctx = nat.context()
    with ctx.lock:
        assert nat.lib().hb_prove_mixed(ctx.h, None, 3, 0) == HB_EINVAL
    valid()


# ------------------------------------------------------------------ 13: PySwizzle.prove_mixed / verify_mixed
def test_pyswizzle_prove_and_verify_mixed(nat, pys, tmp_path):
    rng = np.random.default_rng(130)
    beats = [pys.PySwizzle(16, b"a" * 32, P256), pys.PySwizzle(10, b"b" * 32, recorded_prime(1024, 3024)),
             pys.PySwizzle(3, b"c" * 32, recorded_prime(61, 2061))]
    datas = [[_bytes(rng, int(n)) for n in rng.integers(1, 9000, 3)] for _ in beats]
    encs = [b.encode_many([io.BytesIO(x) for x in ds]) for b, ds in zip(beats, datas)]
    items, vitems = [], []
    files = []
    for k in range(3):                                            # beats interleaved
        for b, (beat, ds, enc) in enumerate(zip(beats, datas, encs)):
            tag, state = enc[k]
            f = io.BytesIO(ds[k])
            if (k, b) == (1, 1):
                path = tmp_path / "f.bin"
                path.write_bytes(ds[k])
                f = open(str(path), "rb")
                files.append(f)
                f.seek(3)
            elif (k, b) == (0, 2):
                f.seek(7)
            chal = beat.gen_challenge(state)
            if (k, b) == (2, 0):
                chal.chunks = 0
            items.append((beat.get_public(), f, chal, tag))
            vitems.append((beat, chal, state))
    try:
        want = [b.prove(f, c, t) for b, f, c, t in items]
        got = pys.PySwizzle.prove_mixed(items)
        assert [(g.mu, g.sigma) for g in got] == [(x.mu, x.sigma) for x in want]
        assert got[6].mu == [0] * 16 and got[6].sigma == 0
        assert items[2][1].tell() == 7 and files[0].tell() == 3
    finally:
        for f in files:
            f.close()
    n = len(items)
    vit = [(beat, g, chal, state) for (beat, chal, state), g in zip(vitems, got)]
    assert pys.PySwizzle.verify_mixed(vit) == [True] * n
    got[4].mu[1] ^= 1                                             # one mu flipped: only that item False
    assert pys.PySwizzle.verify_mixed(vit) == [k != 4 for k in range(n)]
    got[4].mu[1] ^= 1
    # one encrypted state under a wrong beat key: the loop's error
    state = vit[5][3]
    state.encrypt(vit[5][0].key)
    bad = list(vit)
    bad[5] = (vit[3][0],) + vit[5][1:]
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.verify_mixed(bad)
    with pytest.raises(HeartbeatError) as e1:
        [b.verify(pr, c, s) for b, pr, c, s in bad]
    assert str(e.value) == str(e1.value) == "Signature invalid on state."
    assert pys.PySwizzle.verify_mixed(vit) == [True] * n
