"""GPU parity of the batched verify (hb_verify_rhs_many, PySwizzle.verify_many):
the right-hand sides of many small proofs, each under its own f_key, alpha_key
and challenge key, in one PRF launch and one sum launch (hb_vbatch.hpp;
hb_runtime.cpp verify_many_impl).

Every comparison is byte for byte, the batch against hb_verify_rhs per proof;
in addition the CPU oracle's verify accepts that right-hand side as sigma and
rejects it with one bit flipped.  Over

* the wave-job boundaries of `chunks` (0, 1, 15, 16, 17, 33, 255 .. 257, 1000),
  index ranges from 1 to above 2^40, S from 1 to 40 (alpha over three wave-jobs),
* every limb count and AES key size, key_len != chal_key_len (fall-through),
* distinct keys per proof, v_max other than p, more wave-jobs than the chip
  has wave positions,
* group splitting and the fall-through of a long challenge ($HB_TEST_BATCH_CHUNKS),
* encode_many -> prove -> the batch, the context afterwards, errors.

A v_max wider than the prime's limb count is rejected by hb_verify_rhs itself
(HB_EUNSUPPORTED, before its verify_impl), so the batch rejects it with the
same code: the rule for descriptors the single call rejects.

Reference: a caller's loop over PySwizzle.py:372-395."""
import ctypes
import importlib
import io

import numpy as np
import pytest

from test_gpu_parity import P256
from test_gpu_encode_many import _prime, encode_many, encode_single, oracle_raw

pytestmark = pytest.mark.gpu

HB_EINVAL = -1


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


def _mub(p, mu, w):
    return b"".join((int(m) % p).to_bytes(w, "big") for m in mu)


def verify_many(nat, p, S, items, klen=None, cklen=None, flags=0, fill=0xA5):
    """hb_verify_rhs_many over items (f_key, alpha_key, state_chunks, chal_key,
    chunks, v_max, mu ints): (rc, [rhs bytes per proof])."""
    ctx = nat.context()
    n = len(items)
    w = nat.width_of(p)
    descs = (nat.VerifyDesc * max(n, 1))()
    out = np.full(max(n, 1) * w, fill, dtype=np.uint8)
    keep = []
    for i, (fk, ak, nstate, ck, chunks, vmax, mu) in enumerate(items):
        vb, mb = nat.be(vmax), _mub(p, mu, w)
        keep.append((vb, mb))
        d = descs[i]
        d.f_key, d.alpha_key, d.chal_key = fk, ak, ck
        d.state_chunks, d.chunks = nstate, chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.mu = mb
        d.rhs_out = out.ctypes.data + i * w
    pb = nat.be(p)
    klen = (len(items[0][0]) if n else 32) if klen is None else klen
    cklen = (len(items[0][3]) if n else 32) if cklen is None else cklen
    with ctx.lock:
        rc = nat.lib().hb_verify_rhs_many(ctx.h, pb, len(pb), S, klen, cklen, descs, n, flags)
    raw = out.tobytes()
    return rc, [raw[i * w:(i + 1) * w] for i in range(n)]


def verify_single(nat, p, S, item):
    """One hb_verify_rhs: (rc, rhs bytes)."""
    fk, ak, nstate, ck, chunks, vmax, mu = item
    ctx = nat.context()
    w = nat.width_of(p)
    rhs = ctypes.create_string_buffer(w)
    pb, vb = nat.be(p), nat.be(vmax)
    with ctx.lock:
        rc = nat.lib().hb_verify_rhs(ctx.h, pb, len(pb), S, fk, ak, len(fk), nstate, ck, len(ck), chunks,
                                     vb, len(vb), _mub(p, mu, w), rhs)
    return rc, rhs.raw


def last_error(nat):
    return nat.lib().hb_last_error(nat.context().h).decode("utf-8", "replace")


def oracle_checks(oracle, p, S, item, rhs):
    fk, ak, nstate, ck, chunks, vmax, mu = item
    sigma = int.from_bytes(rhs, "big")
    mu = [int(m) % p for m in mu]
    assert sigma < p
    assert oracle.verify(p, S, fk, ak, nstate, ck, chunks, vmax, mu, sigma)
    assert not oracle.verify(p, S, fk, ak, nstate, ck, chunks, vmax, mu, sigma ^ 1)


def check_batch(nat, oracle, p, S, items, **kw):
    """Batch == single per proof, and the oracle's verify agrees."""
    rc, got = verify_many(nat, p, S, items, **kw)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        rc1, one = verify_single(nat, p, S, it)
        assert rc1 == 0, last_error(nat)
        assert got[i] == one, (i, it[2], it[4])
        oracle_checks(oracle, p, S, it, one)
    return got


def _item(rng, p, S, nstate, chunks, vmax=None, klen=32, cklen=None):
    cklen = klen if cklen is None else cklen
    w = (p.bit_length() + 7) // 8
    key = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731
    mu = [int.from_bytes(key(w), "big") % p for _ in range(S)]
    return (key(klen), key(klen), nstate, key(cklen), chunks, p if vmax is None else vmax, mu)


# ------------------------------------------------------------------ 1: shapes
CHUNKS = [0, 1, 15, 16, 17, 33, 255, 256, 257, 1000]
NSTATE = [1, 2, 820, (1 << 27) + 1, (1 << 40) + 3]
_sweeps = {}


def sweep(nat, oracle, S):
    """Test 1's batch for S, checked once: (items, rhs bytes per proof)."""
    if S not in _sweeps:
        rng = np.random.default_rng(100 + S)
        items = [_item(rng, P256, S, ns, n) for n in CHUNKS for ns in NSTATE]
        _sweeps[S] = (items, check_batch(nat, oracle, P256, S, items))
    return _sweeps[S]


@pytest.mark.parametrize("S", [1, 10, 17, 40])
def test_shape_sweep(nat, oracle, S):
    items, got = sweep(nat, oracle, S)
    assert len(got) == 50 and len(items) == 50


# ------------------------------------------------------------------ 2: limbs, key sizes
@pytest.mark.parametrize("bits,S,klen,cklen", [
    (16, 3, 16, 16),       # AES-128
    (256, 1, 24, 24),      # AES-192
    (384, 5, 32, 32),
    (512, 16, 32, 32),
    (1024, 10, 32, 32),    # PySwizzle's defaults
    (2048, 4, 32, 32),     # 64 limbs
    (256, 4, 16, 32),      # state and challenge keys with different round counts: the single verify
])
def test_limb_counts_and_key_sizes(nat, oracle, bits, S, klen, cklen):
    p = P256 if bits == 256 else _prime(bits, 7 * bits + S)
    rng = np.random.default_rng(bits + S + cklen)
    items = [_item(rng, p, S, ns, n, klen=klen, cklen=cklen) for n, ns in [(0, 5), (1, 1), (17, 3000), (40, 1 << 33)]]
    check_batch(nat, oracle, p, S, items)


# ------------------------------------------------------------------ 3: keys stay with their proof
def test_keys_stay_with_their_proof(nat, oracle):
    S = 4
    rng = np.random.default_rng(3)
    base = _item(rng, P256, S, 820, 20)
    key = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()   # noqa: E731
    a = [(key(), key()) + base[2:] for _ in range(33)]                  # equal mu and challenge
    b = [base[:3] + (key(),) + base[4:] for _ in range(33)]             # equal state keys
    for items in (a, b):
        got = check_batch(nat, oracle, P256, S, items)
        assert len(set(got)) == 33


# ------------------------------------------------------------------ 4: v_max other than p
def test_vmax_values(nat, oracle):
    S = 3
    rng = np.random.default_rng(4)
    vmaxes = [2, 255, (1 << 64) + 13, P256 - 1, (1 << 256) - 1]         # the last: above p, inside its limbs
    items = [_item(rng, P256, S, 820, n, vmax=v) for v in vmaxes for n in (1, 37)]
    got = check_batch(nat, oracle, P256, S, items)
    # wider than the prime's limb count: hb_verify_rhs rejects it, so does the batch
    wide = _item(rng, P256, S, 820, 5, vmax=(1 << 256) + 1)
    rc1, _ = verify_single(nat, P256, S, wide)
    assert rc1 == nat.HB_EUNSUPPORTED
    rc, out = verify_many(nat, P256, S, items[:3] + [wide] + items[3:])
    assert rc == nat.HB_EUNSUPPORTED
    assert "proof 3" in last_error(nat)
    assert all(set(o) == {0xA5} for o in out)                           # before any work
    rc, again = verify_many(nat, P256, S, items)
    assert rc == 0 and again == got


# ------------------------------------------------------------------ 5: more wave-jobs than positions
def test_more_wave_jobs_than_wave_positions(nat, oracle):
    rng = np.random.default_rng(5)
    items = [_item(rng, P256, 1, 7 + i, 3) for i in range(5000)]         # 15,000 wave-jobs
    rc, got = verify_many(nat, P256, 1, items)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        rc1, one = verify_single(nat, P256, 1, it)
        assert rc1 == 0 and got[i] == one, i
        oracle_checks(oracle, P256, 1, it, one)


# ------------------------------------------------------------------ 6: HB_TEST_BATCH_CHUNKS
def test_group_splitting(nat, oracle, monkeypatch):
    items, want = sweep(nat, oracle, 10)
    total = sum(CHUNKS) * len(NSTATE)
    cap = 2000
    assert max(CHUNKS) <= cap and 4 * cap < total      # no proof falls through, at least five groups
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", str(cap))
    try:
        rc, got = verify_many(nat, P256, 10, items)
        launches = nat.context().last_kernel_ms()[1]
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want
    assert launches >= 10                               # two launches per group


def test_long_challenge_falls_through(nat, oracle, monkeypatch):
    items, want = sweep(nat, oracle, 10)
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "100")   # the proofs of 255 .. 1000 chunks: the single verify
    try:
        rc, got = verify_many(nat, P256, 10, items)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want


# ------------------------------------------------------------------ 7: encode_many -> prove -> batch
S7 = 16


def prove(nat, p, S, ck, chunks, tags, data):
    """hb_prove over host buffers: (mu ints, sigma int)."""
    ctx = nat.context()
    w = nat.width_of(p)
    mu, sg = ctypes.create_string_buffer(S * w), ctypes.create_string_buffer(w)
    pb = nat.be(p)
    t, d = np.frombuffer(tags, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)
    with ctx.lock:
        ctx.check(nat.lib().hb_prove(ctx.h, pb, len(pb), S, ck, len(ck), chunks, pb, len(pb), t.ctypes.data,
                                     len(tags) // w, d.ctypes.data, len(data), 0, mu, sg))
    return [int.from_bytes(mu.raw[j * w:(j + 1) * w], "big") for j in range(S)], int.from_bytes(sg.raw, "big")


def test_end_to_end(nat, oracle):
    rng = np.random.default_rng(7)
    datas = [rng.integers(0, 256, 3072, dtype=np.uint8).tobytes() for _ in range(3)]
    key = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()   # noqa: E731
    keys = [(key(), key()) for _ in range(3)]
    rc, tags, _ = encode_many(nat, P256, S7, keys, datas)
    assert rc == 0
    w = nat.width_of(P256)
    items, sigmas = [], []
    for (fk, ak), data, tg in zip(keys, datas, tags):
        ck, n = key(), len(tg) // w
        mu, sigma = prove(nat, P256, S7, ck, 2 * n, tg, data)
        items.append((fk, ak, n, ck, 2 * n, P256, mu))
        sigmas.append(sigma)
    rc, got = verify_many(nat, P256, S7, items)
    assert rc == 0, last_error(nat)
    assert [int.from_bytes(g, "big") for g in got] == sigmas
    bad = list(items)
    bad[2] = bad[2][:6] + ([m ^ (1 if j == 5 else 0) for j, m in enumerate(bad[2][6])],)
    rc, got2 = verify_many(nat, P256, S7, bad)
    assert rc == 0
    assert got2[:2] == got[:2] and got2[2] != got[2]


# ------------------------------------------------------------------ 8: the context afterwards
def test_context_left_clean(nat, oracle):
    S = 10
    rng = np.random.default_rng(8)
    items = [_item(rng, P256, S, 820, n) for n in (0, 5, 40, 300)]
    first = check_batch(nat, oracle, P256, S, items)        # batch, then fused verifies (the singles)
    data = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    fk, ak, ck = items[0][0], items[0][1], items[0][3]
    w = nat.width_of(P256)
    tags, _ = encode_single(nat, P256, S, fk, ak, data)      # a plain hb_encode
    assert tags == oracle_raw(oracle, P256, S, fk, ak, data, w)
    n = len(tags) // w
    mu, sigma = prove(nat, P256, S, ck, 50, tags, data)       # a prove, and its verify
    assert (mu, sigma) == tuple(oracle.prove(P256, S, ck, 50, P256, [int.from_bytes(tags[i * w:(i + 1) * w], "big")
                                                                      for i in range(n)], data))
    rc, rhs = verify_single(nat, P256, S, (fk, ak, n, ck, 50, P256, mu))
    assert rc == 0 and int.from_bytes(rhs, "big") == sigma
    rc, many, _ = encode_many(nat, P256, S, [(fk, ak), (ak, fk)], [data, data[:777]])
    assert rc == 0
    assert many[0] == tags and many[1] == oracle_raw(oracle, P256, S, ak, fk, data[:777], w)
    rc, again = verify_many(nat, P256, S, items)
    assert rc == 0 and again == first
    rc, e2e = verify_many(nat, P256, S, [(fk, ak, n, ck, 50, P256, mu)])
    assert rc == 0 and int.from_bytes(e2e[0], "big") == sigma


# ------------------------------------------------------------------ 9: errors, no-ops
def test_errors_and_noops(nat, oracle):
    S = 4
    rng = np.random.default_rng(9)
    items = [_item(rng, P256, S, 50, n) for n in (3, 20)]
    want = check_batch(nat, oracle, P256, S, items)

    def valid():
        rc, got = verify_many(nat, P256, S, items)
        assert rc == 0 and got == want

    rc, got = verify_many(nat, P256, S, [])
    assert rc == 0 and got == []
    rc, got = verify_many(nat, P256, S, items, flags=1)
    assert rc == nat.HB_EUNSUPPORTED
    assert all(set(g) == {0xA5} for g in got)
    valid()
    for klen, cklen in ((15, 32), (32, 17)):
        rc, got = verify_many(nat, P256, S, items, klen=klen, cklen=cklen)
        assert rc == HB_EINVAL
        assert all(set(g) == {0xA5} for g in got)
        valid()
    bad = [items[0], items[1][:2] + (0,) + items[1][3:]]    # state_chunks == 0 with chunks > 0
    assert verify_single(nat, P256, S, bad[1])[0] == HB_EINVAL
    rc, got = verify_many(nat, P256, S, bad)
    assert rc == HB_EINVAL and "proof 1" in last_error(nat)
    assert all(set(g) == {0xA5} for g in got)
    valid()
    rc, got = verify_many(nat, P256, 0, items)
    assert rc == HB_EINVAL
    valid()


# ------------------------------------------------------------------ 10: PySwizzle.verify_many
def test_pyswizzle_verify_many(nat, pys):
    rng = np.random.default_rng(10)
    datas = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 20000, 6)]
    beat = pys.PySwizzle(S7, b"k" * 32, P256)
    pub = beat.get_public()
    items = []
    for x, (tag, state) in zip(datas, beat.encode_many([io.BytesIO(x) for x in datas])):
        chal = beat.gen_challenge(state)
        items.append((pub.prove(io.BytesIO(x), chal, tag), chal, state))
    items[4][0].mu[3] ^= 1
    want = [beat.verify(*it) for it in items]
    assert want == [True, True, True, True, False, True]
    assert beat.verify_many(items) == want
