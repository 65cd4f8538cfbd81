"""GPU parity of the batched cxx verify (hb_cxx_verify_rhs_many,
Swizzle.verify_many of the cxx Swizzle = heartbeat.Heartbeat): the right-hand
sides of many proofs, each under its own f_key, alpha_key and challenge key,
in one lane-engine PRF launch (hb_cpv.hpp) and one sum launch per group
(hb_runtime.cpp cxx_verify_many_impl).

For every proof the batch's rhs == hb_cxx_verify_rhs's, byte for byte, and ==
the restatement below of cxx/shacham_waters_private.cxx:791-842 over the
oracle's cxx prf (the oracle has no cxx verify):
    rhs = sum_i v_i F(idx_i) + sum_j alpha_j mu_j mod p
with idx_i = i when chunks >= state_chunks (check_all, :822-827).  Shapes as in
test_gpu_cxx_prove_many.py, plus state_chunks of 2^24 and 2^32 - 1 (ByteCount
4), key_len and chal_key_len of different AES round counts (everything falls
through), and the Python layer: encode -> prove_many -> verify_many accepts,
and rejects after one flipped file byte.

PARITY UNPINNED as in test_gpu_cxx.py."""
import ctypes
import io
import os

import numpy as np
import pytest

from test_gpu_cxx import P1024
from test_gpu_cxx_prove_many import (HB_CB_JOB, HB_EINVAL, last_error, launches, make_items, other_calls, prime,
                                     prove_many)
from test_gpu_cxx_prove_many import nat, pys, swz  # noqa: F401 -- fixtures
from test_gpu_parity import P256

pytestmark = pytest.mark.gpu

J = HB_CB_JOB
S2 = 2


class Item(object):
    def __init__(self, fk, ak, ck, nstate, chunks, vmax, mu):
        self.fk, self.ak, self.ck = fk, ak, ck
        self.nstate, self.chunks, self.vmax, self.mu = nstate, chunks, vmax, mu


def make(p, S, seed, specs, klen=32, cklen=None, vmax=None):
    """Seeded items from (state_chunks, chunks): keys and random mu values below p."""
    rng = np.random.default_rng(seed)
    w = (p.bit_length() + 7) // 8
    key = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()   # noqa: E731
    out = []
    for nstate, chunks in specs:
        mu = [int.from_bytes(key(w), "big") % p for _ in range(S)]
        out.append(Item(key(klen), key(klen), key(klen if cklen is None else cklen), nstate, chunks,
                        p if vmax is None else vmax, mu))
    return out


def _be(n):
    return n.to_bytes(max(1, (n.bit_length() + 7) // 8), "big")


def _mub(p, it):
    w = (p.bit_length() + 7) // 8
    return b"".join(m.to_bytes(w, "big") for m in it.mu)


def verify_many(nat, p, S, items, flags=0, klen=None, cklen=None, edit=None, fill=0xA5):
    """hb_cxx_verify_rhs_many: (rc, [rhs bytes per item])."""
    ctx = nat.context()
    n = len(items)
    w = nat.width_of(p)
    descs = (nat.VerifyDesc * max(n, 1))()
    out = np.full(max(n, 1) * w, fill, dtype=np.uint8)
    for i, it in enumerate(items):
        d = descs[i]
        vb = _be(it.vmax)
        d.f_key, d.alpha_key, d.chal_key = it.fk, it.ak, it.ck
        d.state_chunks, d.chunks = it.nstate, it.chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.mu = _mub(p, it)
        d.rhs_out = out.ctypes.data + i * w
    if edit is not None:
        edit(descs)
    if klen is None:
        klen = len(items[0].fk) if n else 32
    if cklen is None:
        cklen = len(items[0].ck) if n else 32
    pb = nat.be(p)
    with ctx.lock:
        rc = nat.lib().hb_cxx_verify_rhs_many(ctx.h, pb, len(pb), S, klen, cklen, descs, n, flags)
    raw = out.tobytes()
    return rc, [raw[i * w:(i + 1) * w] for i in range(n)]


def verify_single(nat, p, S, it):
    ctx = nat.context()
    w = nat.width_of(p)
    rhs = ctypes.create_string_buffer(w)
    pb, vb = nat.be(p), _be(it.vmax)
    with ctx.lock:
        rc = nat.lib().hb_cxx_verify_rhs(ctx.h, pb, len(pb), S, it.fk, it.ak, len(it.fk), it.nstate, it.ck,
                                         len(it.ck), it.chunks, vb, len(vb), _mub(p, it), rhs)
    return rc, rhs.raw


def restate(oracle, p, S, it):
    """cxx/shacham_waters_private.cxx:791-842 over oracle.cxx_prf_eval."""
    check_all = it.chunks >= it.nstate
    n = it.nstate if check_all else it.chunks
    acc = 0
    for i in range(n):
        idx = i if check_all else oracle.cxx_prf_eval(it.ck, it.nstate, i)[0]
        acc += oracle.cxx_prf_eval(it.ck, it.vmax, i)[0] * oracle.cxx_prf_eval(it.fk, p, idx)[0]
    for j in range(S):
        acc += oracle.cxx_prf_eval(it.ak, p, j)[0] * it.mu[j]
    return (acc % p).to_bytes((p.bit_length() + 7) // 8, "big")


def check_batch(nat, oracle, p, S, items, use_oracle=True, batched=None, **kw):
    """Batch == loop of the single call (== the restatement) for every item;
    batched: whether the call was one group of two launches, or made the
    launches of the single calls and no other."""
    rc, got = verify_many(nat, p, S, items, **kw)
    assert rc == 0, last_error(nat)
    n, singles = launches(nat), 0
    for i, it in enumerate(items):
        rc1, one = verify_single(nat, p, S, it)
        singles += launches(nat)
        assert rc1 == 0, last_error(nat)
        assert got[i] == one, (i, it.nstate, it.chunks)
        if use_oracle:
            assert got[i] == restate(oracle, p, S, it), (i, it.nstate, it.chunks)
    if batched is not None:
        assert n == (2 if batched else singles)
    return got


# ------------------------------------------------------------------ 1: primes, key sizes, sectors
@pytest.mark.parametrize("bits,S,klen", [
    (256, 16, 16),
    (256, 1, 24),
    (384, 3, 32),
    (1024, 10, 32),    # the cxx Swizzle's defaults
    (1024, 3, 16),
    (2048, 3, 24),
    (257, 4, 32),      # ByteCount 33: every item through hb_cxx_verify_rhs
])
def test_primes_key_sizes(nat, oracle, bits, S, klen):
    p = prime(bits, 7 * bits + S)
    specs = [(1, 1), (1, 6), (2, 1), (4, 3), (4, 4), (10, 7), (10, 2 ** 32 - 1), (21, 21), (21, 6), (5, 0), (0, 0)]
    check_batch(nat, oracle, p, S, make(p, S, bits + S, specs, klen), batched=bits != 257)


def test_mixed_round_counts_fall_through(nat, oracle):
    """key_len 32 with chal_key_len 16: NR is a template parameter of the kernel."""
    specs = [(10, 7), (10, 10), (300, 70), (5, 0)]
    check_batch(nat, oracle, P256, S2, make(P256, S2, 21, specs, klen=32, cklen=16), batched=False)


# ------------------------------------------------------------------ 2: chunk counts, check_all boundary
COUNTS = (0, 1, J - 1, J, J + 1, 4 * J + 1)


@pytest.fixture(scope="module")
def batch2(nat, oracle):
    specs = [(4 * J + 40, n) for n in COUNTS] + [(n, n) for n in COUNTS if n] + [(n, n + 5) for n in COUNTS if n]
    items = make(P256, S2, 2, specs)
    return items, check_batch(nat, oracle, P256, S2, items)


def test_chunk_counts_around_a_wave_job(batch2):
    assert len(batch2[1]) == 3 * len(COUNTS) - 2


def test_check_all_boundary(nat, oracle):
    items = make(P256, S2, 3, [(300, n) for n in (299, 300, 305, 2 ** 32 - 1)])
    for it in items[1:]:
        it.fk, it.ak, it.ck, it.mu = items[0].fk, items[0].ak, items[0].ck, items[0].mu
    got = check_batch(nat, oracle, P256, S2, items)
    assert got[1] == got[2] == got[3] != got[0]


def test_check_all_1024(nat, oracle):
    specs = [(21, 21), (21, 6), (J, J), (J + 1, J + 2), (3, 1), (820, 246)]
    check_batch(nat, oracle, P1024, 10, make(P1024, 10, 4, specs))


# ------------------------------------------------------------------ 3: index widths
def test_index_widths(nat, oracle):
    """ByteCount(state_chunks) 1 to 4."""
    specs = [(n, min(40, n - 1)) for n in (1, 5, 255, 256, 257, 65535, 65536, 70000, 1 << 24, 2 ** 32 - 1)]
    check_batch(nat, oracle, P256, 1, make(P256, 1, 5, specs))
    # past 2^32 - 1 blocks: as hb_cxx_verify_rhs
    items = make(P256, 1, 5, [(5, 3), (1 << 32, 3)])
    rc, got = verify_many(nat, P256, 1, items)
    assert rc == nat.HB_EUNSUPPORTED and "proof 1" in last_error(nat)
    assert verify_single(nat, P256, 1, items[1])[0] == nat.HB_EUNSUPPORTED
    assert all(set(g) == {0xA5} for g in got)


# ------------------------------------------------------------------ 4: v_max
def test_v_max(nat, oracle):
    items = []
    for k, vm in enumerate([P256, (1 << 127) + 45, (1 << 256) - 189, (1 << 39) + 7]):
        items += make(P256, S2, 40 + k, [(100, 30), (10, 10)], vmax=vm)
    check_batch(nat, oracle, P256, S2, items)
    assert verify_single(nat, P256, S2, items[6])[0] == 0
    a = launches(nat)
    assert verify_single(nat, P256, S2, items[7])[0] == 0
    b = launches(nat)
    rc, _ = verify_many(nat, P256, S2, items)
    assert rc == 0 and launches(nat) == 2 + a + b


# ------------------------------------------------------------------ 5: item sets
def test_items_that_differ_only_in_the_challenge_key(nat, oracle):
    items = make(P256, S2, 6, [(100, 20)] * 33)
    for it in items:
        it.fk, it.ak, it.mu = items[0].fk, items[0].ak, items[0].mu
    items[32].ck = items[0].ck
    got = check_batch(nat, oracle, P256, S2, items)
    assert got[0] == got[32] and len(set(got[:32])) == 32


def test_600_items_of_30_chunks(nat):
    check_batch(nat, None, P256, S2, make(P256, S2, 7, [(50, 30)] * 600), use_oracle=False)


def test_5000_one_chunk_items(nat, oracle):
    items = make(P256, S2, 8, [(4, 1), (1, 1)] * 2500, klen=16)
    rc, got = verify_many(nat, P256, S2, items)
    assert rc == 0, last_error(nat)
    for i in list(range(0, 5000, 97)) + [4999]:
        assert got[i] == restate(oracle, P256, S2, items[i]), i
        assert verify_single(nat, P256, S2, items[i]) == (0, got[i]), i


# ------------------------------------------------------------------ 6: splitting, fall-through
def test_group_splitting_and_fall_through(nat, oracle, monkeypatch):
    """Seven proofs, cap 20 chunks: six of 10 effective chunks make three
    groups of two launches each, the one of 50 goes through hb_cxx_verify_rhs."""
    specs = [(100, 10), (10, 10), (100, 50), (100, 10), (10, 11), (100, 10), (100, 10)]
    items = make(P256, S2, 12, specs)
    want = check_batch(nat, oracle, P256, S2, items)
    assert verify_single(nat, P256, S2, items[2]) == (0, want[2])
    single_launches = launches(nat)
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "20")
    try:
        rc, got = verify_many(nat, P256, S2, items)
        n = launches(nat)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0 and got == want
    rc, got = verify_many(nat, P256, S2, items)
    assert rc == 0 and got == want and launches(nat) == 2      # one group: PRF, sum
    assert n == 3 * 2 + single_launches


# ------------------------------------------------------------------ 7: errors, then a valid batch
def test_errors_then_a_valid_batch(nat, oracle):
    items = make(P256, S2, 13, [(100, 10), (1, 1), (6, 6), (13, 5), (9, 0)])
    want = check_batch(nat, oracle, P256, S2, items)
    untouched = lambda got: all(set(g) == {0xA5} for g in got)   # noqa: E731

    def valid():
        rc, got = verify_many(nat, P256, S2, items)
        assert rc == 0 and got == want

    def setf(field, value):
        return lambda descs: setattr(descs[3], field, value)

    def vmax(v):
        def f(descs):
            descs[3].vmax_be, descs[3].vmax_len = v, len(v)
        return f

    for field in ("f_key", "alpha_key", "chal_key", "mu", "rhs_out", "vmax_be"):
        rc, got = verify_many(nat, P256, S2, items, edit=setf(field, None))
        assert rc == HB_EINVAL and "proof 3" in last_error(nat), field
        assert untouched(got)
        valid()
    rc, got = verify_many(nat, P256, S2, items, edit=setf("state_chunks", 0))
    assert rc == HB_EINVAL and "proof 3: state has no chunks" in last_error(nat) and untouched(got)
    valid()
    rc, got = verify_many(nat, P256, S2, items, edit=vmax(b"\0\0"))
    assert rc == HB_EINVAL and "proof 3: v_max must be positive" in last_error(nat) and untouched(got)
    valid()
    rc, got = verify_many(nat, P256, S2, items, edit=vmax(b"\x01" + b"\0" * 32))
    assert rc == nat.HB_EUNSUPPORTED and "proof 3" in last_error(nat) and untouched(got)
    valid()
    for kw in ({"klen": 15}, {"cklen": 33}):
        rc, got = verify_many(nat, P256, S2, items, **kw)
        assert rc == HB_EINVAL and untouched(got)
    rc, got = verify_many(nat, P256, 0, items)
    assert rc == HB_EINVAL and untouched(got)
    valid()
    for flags in (1, 2, nat.HB_PRF_CXX, nat.HB_ASYNC, 1 << 20):
        rc, got = verify_many(nat, P256, S2, items, flags=flags)
        assert rc == nat.HB_EUNSUPPORTED and untouched(got), flags
    valid()
    rc, got = verify_many(nat, P256, S2, [])
    assert rc == 0 and got == []
    valid()


# ------------------------------------------------------------------ 8: the context afterwards
def test_context_afterwards(nat, oracle, pys, swz, batch2, monkeypatch):
    """After both new calls: a fused prove, a fused verify, a two-pass encode
    and the four existing batches, each equal to what it gave before; then the
    new calls again and the single cxx verify."""
    items, want = batch2
    pitems = make_items(P256, S2, 14, [(99 * 64 + 5, 30), (9 * 64, 10), (5, 1)])
    rc, pwant = prove_many(nat, P256, S2, pitems)
    assert rc == 0
    before = other_calls(nat, pys, swz, monkeypatch)
    assert verify_many(nat, P256, S2, items) == (0, want)
    assert prove_many(nat, P256, S2, pitems) == (0, pwant)
    assert other_calls(nat, pys, swz, monkeypatch) == before
    assert verify_many(nat, P256, S2, items) == (0, want)
    assert prove_many(nat, P256, S2, pitems) == (0, pwant)
    assert verify_single(nat, P256, S2, items[3]) == (0, want[3])


# ------------------------------------------------------------------ 9: the Python layer
def test_heartbeat_prove_many_verify_many(nat, swz, tmp_path):
    """heartbeat.Heartbeat(): encode_many -> prove_many -> verify_many equals
    the loops of prove() and verify() at check_fraction 1.0 and 0.3, accepts
    every honest proof and rejects the one of a file with a flipped byte."""
    import heartbeat
    assert heartbeat.Heartbeat is swz.Swizzle
    rng = np.random.default_rng(9)
    C = 128 * 10
    datas = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (0, 1, C, 3 * C + 5, 20000, 70000)]
    beat = heartbeat.Heartbeat(prime=P1024)
    pub = beat.get_public()
    enc = beat.encode_many([io.BytesIO(x) for x in datas])
    path = tmp_path / "f5.bin"
    path.write_bytes(datas[5])
    for fraction in (1.0, 0.3):
        beat.check_fraction = fraction
        chals = [beat.gen_challenge(state) for _, state in enc]
        files = [io.BytesIO(x) for x in datas[:5]] + [open(str(path), "rb")]
        try:
            files[4].seek(123)
            files[5].seek(77)
            proofs = pub.prove_many([(f, c, tag) for f, c, (tag, _) in zip(files, chals, enc)])
            assert files[4].tell() == 123 and files[5].tell() == 77          # positions restored
        finally:
            files[5].close()
        loop = [pub.prove(io.BytesIO(x), c, tag) for x, c, (tag, _) in zip(datas, chals, enc)]
        assert [(q.mu, q.sigma) for q in proofs] == [(q.mu, q.sigma) for q in loop], fraction
        items = [(q, c, state) for q, c, (_, state) in zip(proofs, chals, enc)]
        assert beat.verify_many(items) == [beat.verify(*it) for it in items] == [True] * len(datas), fraction
    beat.check_fraction = 1.0
    chals = [beat.gen_challenge(state) for _, state in enc]
    bad = bytearray(datas[4])
    bad[len(bad) // 2] ^= 1
    tampered = [io.BytesIO(x) for x in datas[:4]] + [io.BytesIO(bytes(bad)), io.BytesIO(datas[5])]
    proofs = pub.prove_many([(f, c, tag) for f, c, (tag, _) in zip(tampered, chals, enc)])
    items = [(q, c, state) for q, c, (_, state) in zip(proofs, chals, enc)]
    items.insert(2, (proofs[0], "not a challenge", enc[0][1]))                   # wrong type: None
    short = swz.Proof()
    short.mu, short.sigma = proofs[1].mu[:-1], proofs[1].sigma
    items.append((short, chals[1], enc[1][1]))                                   # len(mu) != S: False
    want = [True, True, None, True, True, False, True, False]
    assert beat.verify_many(items) == want == [beat.verify(*it) for it in items]
    assert pub.prove_many([]) == [] and beat.verify_many([]) == []
    os.remove(str(path))
