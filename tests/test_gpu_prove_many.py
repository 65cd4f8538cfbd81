"""GPU parity of the batched prove (hb_prove_many, PySwizzle.prove_many): mu and
sigma of many small proofs, each under its own challenge key, file and tag
array, in one PRF launch and one sum launch per group (hb_pbatch.hpp;
hb_runtime.cpp prove_many_impl).

Every comparison is byte for byte: the batch against hb_prove per proof, and
against the CPU oracle's prove.  Over

* the wave-job boundaries of `chunks` (0, 1, 15, 16, 17, 33, 257, 1000) x file
  lengths around the sector and block sizes x tag counts from 1 to past EOF,
  S in 1, 10, 40,
* every limb count (20- to 2048-bit primes) and AES key size,
* the reference's recorded proofs (tests/golden/encode_cases.json),
* factors that are not below p (sectors and tags of 0xFF bytes, v_max > p),
* proofs that differ only in their key or only in their file, more wave-jobs
  than the chip has wave positions,
* device- and host-resident data and tags in all four combinations,
* group splitting and the three fall-throughs (a long challenge, a host file
  that is not uploaded, host data with device tags),
* encode_many -> prove_many -> verify_many, the context afterwards, errors.

Tags are the caller's bytes: most cases use random ones (values up to
2^(8 width) - 1, not reduced mod p), which the single prove and the oracle
take as well.

Reference: a caller's loop over PySwizzle.py:333-370."""
import ctypes
import importlib
import io

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import P256, DevBuf
from test_gpu_encode_many import encode_many, encode_single, oracle_raw
from test_gpu_primes import seeded_prime
from test_gpu_verify_many import verify_many, verify_single

pytestmark = pytest.mark.gpu

HB_EINVAL = -1
PRIMES = load_golden("primes.json")
P256MAX, P255 = int(PRIMES["p256max"], 16), int(PRIMES["p255"], 16)


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


def last_error(nat):
    return nat.lib().hb_last_error(nat.context().h).decode("utf-8", "replace")


def prove_many(nat, p, S, items, flags=0, klen=None, data_ptrs=None, tag_ptrs=None, fill=0xA5):
    """hb_prove_many over items (chal_key, chunks, v_max, tag bytes, file
    bytes): (rc, [(mu bytes, sigma bytes) per proof]).  Host buffers unless
    data_ptrs / tag_ptrs give device addresses."""
    ctx = nat.context()
    n = len(items)
    w = nat.width_of(p)
    descs = (nat.ProveDesc * max(n, 1))()
    out = np.full(max(n, 1) * (S + 1) * w, fill, dtype=np.uint8)
    keep = []
    for i, (ck, chunks, vmax, tags, data) in enumerate(items):
        vb = nat.be(vmax)
        t, a = np.frombuffer(tags, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
        keep.append((vb, t, a))
        d = descs[i]
        d.chal_key, d.chunks = ck, chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.tags = tag_ptrs[i] if tag_ptrs is not None else (t.ctypes.data if len(t) else None)
        d.ntags = len(tags) // w
        d.data = data_ptrs[i] if data_ptrs is not None else (a.ctypes.data if len(a) else None)
        d.len = len(data)
        d.mu_out = out.ctypes.data + i * (S + 1) * w
        d.sigma_out = out.ctypes.data + (i * (S + 1) + S) * w
    pb = nat.be(p)
    klen = (len(items[0][0]) if n else 32) if klen is None else klen
    with ctx.lock:
        rc = nat.lib().hb_prove_many(ctx.h, pb, len(pb), S, klen, descs, n, flags)
    raw = out.tobytes()
    return rc, [(raw[i * (S + 1) * w:(i * (S + 1) + S) * w], raw[(i * (S + 1) + S) * w:(i + 1) * (S + 1) * w])
                for i in range(n)]


def prove_single(nat, p, S, item, flags=0, data_ptr=None, tag_ptr=None):
    """One hb_prove: (rc, (mu bytes, sigma bytes))."""
    ck, chunks, vmax, tags, data = item
    ctx = nat.context()
    w = nat.width_of(p)
    mu, sg = ctypes.create_string_buffer(S * w), ctypes.create_string_buffer(w)
    pb, vb = nat.be(p), nat.be(vmax)
    t, a = np.frombuffer(tags, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
    tp = tag_ptr if tag_ptr is not None else (t.ctypes.data if len(t) else None)
    dp = data_ptr if data_ptr is not None else (a.ctypes.data if len(a) else None)
    with ctx.lock:
        rc = nat.lib().hb_prove(ctx.h, pb, len(pb), S, ck, len(ck), chunks, vb, len(vb), tp, len(tags) // w,
                                dp, len(data), flags, mu, sg)
    return rc, (mu.raw, sg.raw)


def oracle_proof(oracle, p, S, item):
    """The oracle's prove as (mu bytes, sigma bytes)."""
    ck, chunks, vmax, tags, data = item
    w = (p.bit_length() + 7) // 8
    ints = [int.from_bytes(tags[i * w:(i + 1) * w], "big") for i in range(len(tags) // w)]
    mu, sigma = oracle.prove(p, S, ck, chunks, vmax, ints, data)
    return b"".join(m.to_bytes(w, "big") for m in mu), sigma.to_bytes(w, "big")


def check_batch(nat, oracle, p, S, items, single=True, **kw):
    """Batch == hb_prove per proof == the oracle's prove."""
    rc, got = prove_many(nat, p, S, items, **kw)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        if single:
            rc1, one = prove_single(nat, p, S, it)
            assert rc1 == 0, last_error(nat)
            assert got[i] == one, (i, it[1], len(it[3]), len(it[4]))
        assert got[i] == oracle_proof(oracle, p, S, it), (i, it[1], len(it[3]), len(it[4]))
    return got


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _item(rng, p, S, chunks, length, ntags=None, vmax=None, klen=32):
    w = (p.bit_length() + 7) // 8
    C = (p.bit_length() // 8) * S
    ntags = length // C + 1 if ntags is None else ntags
    return (_bytes(rng, klen), chunks, p if vmax is None else vmax, _bytes(rng, ntags * w), _bytes(rng, length))


# ------------------------------------------------------------------ 1: shapes
CHUNKS = [0, 1, 15, 16, 17, 33, 257, 1000]
_sweeps = {}


def sweep(nat, oracle, S):
    """Test 1's batch for S, checked once: (items, results)."""
    if S not in _sweeps:
        rng = np.random.default_rng(200 + S)
        ss, C = 32, 32 * S
        lengths = [0, 1, ss - 1, C - 1, C, C + 1, 3 * C + 17, (64 << 10) + 5]
        items = [_item(rng, P256, S, n, ln, nt)
                 for n in CHUNKS for ln in lengths for nt in (1, ln // C + 1, ln // C + 4)]   # the last: past EOF
        _sweeps[S] = (items, check_batch(nat, oracle, P256, S, items))
    return _sweeps[S]


@pytest.mark.parametrize("S", [1, 10, 40])
def test_shape_sweep(nat, oracle, S):
    items, got = sweep(nat, oracle, S)
    assert len(got) == len(items) == 192
    w = nat.width_of(P256)
    for it, (mu, sg) in zip(items, got):
        if it[1] == 0:
            assert mu == bytes(S * w) and sg == bytes(w)


# ------------------------------------------------------------------ 2: limbs, key sizes
@pytest.mark.parametrize("bits", [20, 61, 129, 256, 257, 512, 1024, 1025, 2048])
def test_limb_counts_and_key_sizes(nat, oracle, bits):
    p = seeded_prime(bits, 2000 + bits)
    S = 3
    C = (bits // 8) * S
    for klen in (16, 24, 32):                       # AES-128, -192, -256: one batch each
        rng = np.random.default_rng(bits + klen)
        items = [_item(rng, p, S, n, ln, klen=klen)
                 for n, ln in [(0, 5), (1, 0), (17, 4 * C + (bits // 8) // 2 + 1), (40, 40 * C + 1), (33, C - 1)]]
        check_batch(nat, oracle, p, S, items)


# ------------------------------------------------------------------ 3: the reference's recorded proofs
def test_golden_proofs(nat, golden_encode):
    groups = {}
    for c in golden_encode["cases"]:
        p = int(c["prime"], 16)
        w = nat.width_of(p)
        tags = b"".join(int(t, 16).to_bytes(w, "big") for t in c["tags"])
        data = bytes.fromhex(c["data"])
        for chn, prn in (("chal", "proof"), ("chal2", "proof2")):
            ch = c[chn]
            want = (b"".join(int(m, 16).to_bytes(w, "big") for m in c[prn]["mu"]), int(c[prn]["sigma"], 16).to_bytes(w, "big"))
            item = (bytes.fromhex(ch["key"]), ch["chunks"], int(ch["v_max"], 16), tags, data)
            groups.setdefault((p, c["sectors"], len(item[0])), []).append((item, want, c["name"]))
    n = 0
    for (p, S, klen), rows in groups.items():
        rc, got = prove_many(nat, p, S, [r[0] for r in rows])
        assert rc == 0, last_error(nat)
        for g, (_, want, name) in zip(got, rows):
            assert g == want, name
            n += 1
    assert n == 352 and len(groups) > 1


# ------------------------------------------------------------------ 4: factors that are not below p
def test_sectors_and_tags_above_p(nat, oracle):
    """bitlen(p) a multiple of 8: a sector of 0xFF bytes is above p, and so is
    a tag of 0xFF bytes."""
    S = 3
    rng = np.random.default_rng(4)
    items = [(_bytes(rng, 32), n, P256MAX, b"\xff" * (32 * nt), b"\xff" * ln)
             for n, ln, nt in [(1, 96, 2), (17, 96 * 5 + 31, 6), (300, 96 * 9, 10)]]
    check_batch(nat, oracle, P256MAX, S, items)


def test_vmax_values(nat, oracle):
    """v_max below, at and above p (inside its limbs): v_i itself may exceed p."""
    S = 3
    rng = np.random.default_rng(5)
    items = [_item(rng, P255, S, n, 1000, vmax=v) for v in (2, P255, (1 << 256) - 1) for n in (1, 37)]
    got = check_batch(nat, oracle, P255, S, items)
    # wider than the prime's limb count: hb_prove rejects it, so does the batch
    wide = _item(rng, P255, S, 5, 1000, vmax=(1 << 256) + 1)
    assert prove_single(nat, P255, S, wide)[0] == nat.HB_EUNSUPPORTED
    rc, out = prove_many(nat, P255, S, items[:3] + [wide] + items[3:])
    assert rc == nat.HB_EUNSUPPORTED and "proof 3" in last_error(nat)
    assert all(set(m) | set(s) == {0xA5} for m, s in out)                # before any work
    rc, again = prove_many(nat, P255, S, items)
    assert rc == 0 and again == got


# ------------------------------------------------------------------ 5: results stay with their proof
def test_results_stay_with_their_proof(nat, oracle):
    S = 4
    rng = np.random.default_rng(6)
    base = _item(rng, P256, S, 20, 3000)
    a = [(_bytes(rng, 32),) + base[1:] for _ in range(33)]              # differ only in the challenge key
    b = [base[:4] + (_bytes(rng, 3000),) for _ in range(33)]            # differ only in the file
    for items in (a, b):
        got = check_batch(nat, oracle, P256, S, items)
        assert len(set(got)) == 33
    assert len({s for _, s in check_batch(nat, oracle, P256, S, b)}) == 1   # one key, one tag array: one sigma


# ------------------------------------------------------------------ 6: more wave-jobs than positions
def test_more_wave_jobs_than_wave_positions(nat, oracle):
    S = 2
    rng = np.random.default_rng(7)
    pool, tags = _bytes(rng, 4000 + 700), _bytes(rng, 32 * 12)
    items = [(_bytes(rng, 32), 17, P256, tags, pool[i:i + 700]) for i in range(4000)]   # 16,000 wave-jobs
    rc, got = prove_many(nat, P256, S, items)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        assert got[i] == oracle_proof(oracle, P256, S, it), i
        if i % 16 == 0:
            rc1, one = prove_single(nat, P256, S, it)
            assert rc1 == 0 and got[i] == one, i


# ------------------------------------------------------------------ 7: residency
@pytest.fixture(scope="module")
def resident(nat, oracle):
    """16 proofs, their host-buffer batch checked once, and the files and tags
    on the device at odd byte offsets."""
    S = 10
    rng = np.random.default_rng(8)
    C = 32 * S
    items = [_item(rng, P256, S, n, ln, nt) for n, ln, nt in
             [(1, 0, 1), (16, C, 2), (17, 3 * C + 17, 7), (33, 20000, None), (257, 65541, None), (40, C - 1, 1),
              (5, 1, 1), (100, 31, 3)] * 2]
    want = check_batch(nat, oracle, P256, S, items)
    doffs, toffs, d, t = [], [], 1, 1
    for it in items:
        doffs.append(d)
        toffs.append(t)
        d = (d + len(it[4]) + 2) | 1
        t = (t + len(it[3]) + 2) | 1
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    for it, do, to in zip(items, doffs, toffs):
        dbuf.upload(it[4], do)
        tbuf.upload(it[3], to)
    yield S, items, want, [dbuf.p + o for o in doffs], [tbuf.p + o for o in toffs]
    dbuf.free()
    tbuf.free()


@pytest.mark.parametrize("flags", [3, 1, 2])
def test_residency(nat, resident, flags):
    """Device data and tags (3), device data with host tags (1: the tags go up
    in the staging copy), host data with device tags (2: the single prove)."""
    S, items, want, dptrs, tptrs = resident
    rc, got = prove_many(nat, P256, S, items, flags=flags, data_ptrs=dptrs if flags & 1 else None,
                         tag_ptrs=tptrs if flags & 2 else None)
    launches = nat.context().last_kernel_ms()[1]
    assert rc == 0, last_error(nat)
    assert got == want
    # one group of PRF, Montgomery and sum launches; the single prove's count otherwise
    assert launches == 3 if flags != 2 else launches <= 2
    if flags == 3:
        for i in (2, 4):
            rc1, one = prove_single(nat, P256, S, items[i], flags=3, data_ptr=dptrs[i], tag_ptr=tptrs[i])
            assert rc1 == 0 and one == want[i]


# ------------------------------------------------------------------ 8: splitting, fall-through
def test_group_splitting(nat, oracle, monkeypatch):
    items, want = sweep(nat, oracle, 10)
    total = sum(it[1] for it in items)
    cap = 4000
    assert max(CHUNKS) <= cap and 6 * cap < total       # no proof falls through, at least seven groups
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", str(cap))
    try:
        rc, got = prove_many(nat, P256, 10, items)
        launches = nat.context().last_kernel_ms()[1]
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want
    assert launches >= 21                                # three launches per group


def test_long_challenge_falls_through(nat, oracle, monkeypatch):
    items, want = sweep(nat, oracle, 10)
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "100")    # the proofs of 257 and 1000 chunks: the single prove
    try:
        rc, got = prove_many(nat, P256, 10, items)
        launches = nat.context().last_kernel_ms()[1]
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want
    assert launches <= 2                                 # the call ended on a single prove


def test_host_file_not_uploaded_falls_through(nat, oracle, resident, monkeypatch):
    """A host file above max(2 chunks C, 8 MiB) is not uploaded whole: the
    single prove gathers its challenged blocks on the host.  And with
    $HB_NO_PROVE_UPLOAD no host file is uploaded at all."""
    S = 2
    rng = np.random.default_rng(9)
    big = (8 << 20) + 1
    small = [_item(rng, P256, S, n, ln) for n, ln in ((17, 5000), (3, 64))]
    items = [small[0], _item(rng, P256, S, 5, big), small[1]]
    got = check_batch(nat, oracle, P256, S, items)
    rc, again = prove_many(nat, P256, S, items)
    assert rc == 0 and again == got
    assert nat.context().last_kernel_ms()[1] <= 2        # the call ended on the single prove of the large file
    rc, alone = prove_many(nat, P256, S, small)
    assert rc == 0 and alone == [got[0], got[2]]
    assert nat.context().last_kernel_ms()[1] == 3
    S2, ritems, want = resident[:3]
    monkeypatch.setenv("HB_NO_PROVE_UPLOAD", "1")
    try:
        rc, got2 = prove_many(nat, P256, S2, ritems)
        launches = nat.context().last_kernel_ms()[1]
    finally:
        monkeypatch.delenv("HB_NO_PROVE_UPLOAD", raising=False)
    assert rc == 0, last_error(nat)
    assert got2 == want and launches <= 2


# ------------------------------------------------------------------ 9: round trip, the context afterwards
def test_round_trip_and_context(nat, oracle):
    S = 16
    rng = np.random.default_rng(10)
    datas = [_bytes(rng, n) for n in (3072, 1, 20000, 512 * 7)]
    keys = [(_bytes(rng, 32), _bytes(rng, 32)) for _ in datas]
    rc, tags, _ = encode_many(nat, P256, S, keys, datas)
    assert rc == 0
    w = nat.width_of(P256)
    items = [(_bytes(rng, 32), 2 * (len(tg) // w), P256, tg, d) for tg, d in zip(tags, datas)]
    proofs = check_batch(nat, oracle, P256, S, items)
    ints = lambda mu: [int.from_bytes(mu[j * w:(j + 1) * w], "big") for j in range(S)]   # noqa: E731
    vitems = [(fk, ak, len(tg) // w, it[0], it[1], P256, ints(mu))
              for (fk, ak), tg, it, (mu, _) in zip(keys, tags, items, proofs)]
    rc, rhs = verify_many(nat, P256, S, vitems)
    assert rc == 0 and rhs == [sg for _, sg in proofs]                    # every proof accepted
    for k in range(len(items)):                                          # and rejected with one bit flipped
        bad = list(vitems)
        bad[k] = bad[k][:6] + ([m ^ (1 if j == k else 0) for j, m in enumerate(bad[k][6])],)
        rc, rhs2 = verify_many(nat, P256, S, bad)
        assert rc == 0 and [a == b for a, b in zip(rhs2, rhs)] == [j != k for j in range(len(items))]
    # the same context afterwards: a fused prove (device-resident, aligned), a
    # fused verify, an encode, and the batch again
    data, tg, it = datas[2], tags[2], items[2]
    dbuf, tbuf = DevBuf(nat, len(data)), DevBuf(nat, len(tg))
    try:
        dbuf.upload(data)
        tbuf.upload(tg)
        rc, one = prove_single(nat, P256, S, (it[0], 40) + it[2:], flags=3, data_ptr=dbuf.p, tag_ptr=tbuf.p)
        assert rc == 0 and nat.context().last_kernel_ms()[1] == 1        # one fused launch
        assert one == oracle_proof(oracle, P256, S, (it[0], 40) + it[2:])
    finally:
        dbuf.free()
        tbuf.free()
    rc, r1 = verify_single(nat, P256, S, vitems[2])
    assert rc == 0 and r1 == proofs[2][1]
    enc, _ = encode_single(nat, P256, S, keys[0][0], keys[0][1], datas[0])
    assert enc == tags[0] == oracle_raw(oracle, P256, S, keys[0][0], keys[0][1], datas[0], w)
    rc, again = prove_many(nat, P256, S, items)
    assert rc == 0 and again == proofs


# ------------------------------------------------------------------ 10: errors, no-ops
def test_errors_and_noops(nat, oracle):
    S = 4
    rng = np.random.default_rng(11)
    items = [_item(rng, P256, S, n, 700) for n in (3, 20, 0)]
    want = check_batch(nat, oracle, P256, S, items)
    untouched = lambda out: all(set(m) | set(s) == {0xA5} for m, s in out)   # noqa: E731

    def valid():
        rc, got = prove_many(nat, P256, S, items)
        assert rc == 0 and got == want

    rc, got = prove_many(nat, P256, S, [])
    assert rc == 0 and got == []
    for flags in (nat.HB_PRF_CXX, nat.HB_ASYNC | 3, nat.HB_ENCODE_SINGLE_PASS, 1 << 20):
        rc, got = prove_many(nat, P256, S, items, flags=flags)
        assert rc == nat.HB_EUNSUPPORTED and untouched(got)
    valid()
    rc, got = prove_many(nat, P256, S, items, klen=15)
    assert rc == HB_EINVAL and untouched(got)
    rc, got = prove_many(nat, P256, 0, items)
    assert rc == HB_EINVAL
    valid()
    # what hb_prove rejects, with its code, also when chunks == 0
    for k, chunks in ((1, 20), (2, 0)):
        for bad, code in (((items[k][0], chunks, P256, b"", items[k][4]), HB_EINVAL),               # ntags == 0
                          ((items[k][0], chunks, 0) + items[k][3:], HB_EINVAL),                    # v_max == 0
                          ((items[k][0], chunks, 1 << 256) + items[k][3:], nat.HB_EUNSUPPORTED)):   # v_max too wide
            assert prove_single(nat, P256, S, bad)[0] == code
            batch = list(items)
            batch[k] = bad
            rc, got = prove_many(nat, P256, S, batch)
            assert rc == code and "proof %d" % k in last_error(nat) and untouched(got)
        valid()
    # NULL buffers
    ctx = nat.context()
    pb = nat.be(P256)
    for field in ("chal_key", "mu_out", "sigma_out", "tags", "data"):
        n, w = len(items), nat.width_of(P256)
        descs = (nat.ProveDesc * n)()
        out = np.full(n * (S + 1) * w, 0xA5, dtype=np.uint8)
        keep = []
        for i, (ck, chunks, vmax, tags, data) in enumerate(items):
            vb, t, a = nat.be(vmax), np.frombuffer(tags, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
            keep.append((vb, t, a))
            d = descs[i]
            d.chal_key, d.chunks, d.vmax_be, d.vmax_len = ck, chunks, vb, len(vb)
            d.tags, d.ntags, d.data, d.len = t.ctypes.data, len(tags) // w, a.ctypes.data, len(data)
            d.mu_out = out.ctypes.data + i * (S + 1) * w
            d.sigma_out = out.ctypes.data + (i * (S + 1) + S) * w
        setattr(descs[1], field, None)
        with ctx.lock:
            rc = nat.lib().hb_prove_many(ctx.h, pb, len(pb), S, 32, descs, n, 0)
        assert rc == HB_EINVAL and "proof 1" in last_error(nat), field
        assert set(out.tobytes()) == {0xA5}
    valid()


# ------------------------------------------------------------------ 11: PySwizzle.prove_many
def test_pyswizzle_prove_many(nat, pys, tmp_path):
    rng = np.random.default_rng(12)
    datas = [_bytes(rng, int(n)) for n in rng.integers(1, 20000, 6)]
    beat = pys.PySwizzle(16, b"k" * 32, P256)
    pub = beat.get_public()
    enc = beat.encode_many([io.BytesIO(x) for x in datas])
    files = [io.BytesIO(x) for x in datas[:4]]
    for k in (4, 5):
        path = tmp_path / ("f%d.bin" % k)
        path.write_bytes(datas[k])
        files.append(open(str(path), "rb"))
    try:
        files[1].seek(7)
        files[5].seek(3)
        chals = [beat.gen_challenge(state) for _, state in enc]
        chals[2].chunks = 0
        items = [(f, ch, tag) for f, ch, (tag, _) in zip(files, chals, enc)]
        want = [pub.prove(*it) for it in items]
        got = pub.prove_many(items)
        assert [(g.mu, g.sigma) for g in got] == [(x.mu, x.sigma) for x in want]
        assert got[2].mu == [0] * 16 and got[2].sigma == 0
        assert files[1].tell() == 7 and files[5].tell() == 3
        states = [state for _, state in enc]
        assert beat.verify_many([(g, ch, st) for g, ch, st in zip(got, chals, states)]) == [True] * 6
    finally:
        for f in files[4:]:
            f.close()
