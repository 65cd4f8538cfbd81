"""GPU parity of the cxx mixed-owner batched verify (hb_cxx_verify_rhs_mixed,
Swizzle.verify_mixed of the cxx Swizzle = heartbeat.Heartbeat): the right-hand
sides of many proofs that each name their own prime, sector count and key
lengths, in two launches per group of a (limb count, AES round count) class
(hb_cmixed.hpp; hb_runtime.cpp cxx_verify_mixed_impl).

For every proof the mixed call's rhs == hb_cxx_verify_rhs's, byte for byte,
and == test_gpu_cxx_verify_many.py's restatement of
cxx/shacham_waters_private.cxx:791-842 over the oracle's cxx prf.  Over alpha
slots of neighbours with different S, every class and key length in one call
with primes that fall through, chunk counts around a wave-job and the
check_all boundary, state_chunks whose ByteCount is 1 to 4, the v_max cases,
key_len and chal_key_len of different round counts, the caps, errors, the
context afterwards, and heartbeat.Heartbeat.prove_mixed / verify_mixed end to
end.

PARITY UNPINNED as in test_gpu_cxx.py."""
import io
import random

import numpy as np
import pytest

from test_gpu_cxx_prove_many import HB_CB_JOB, HB_EINVAL, last_error, launches, other_calls
from test_gpu_cxx_prove_many import nat, pys, swz  # noqa: F401 -- fixtures
from test_gpu_cxx_verify_many import _be, _mub, make, restate, verify_many, verify_single
from test_gpu_parity import P256
from test_gpu_primes import seeded_prime
from test_gpu_prove_mixed import recorded_prime
from test_gpu_verify_mixed import verify_mixed as py_verify_mixed

pytestmark = pytest.mark.gpu

J = HB_CB_JOB
P128 = seeded_prime(128, 2128)
P384 = seeded_prime(384, 2384)
P256B = recorded_prime(256, 2256)
P512 = recorded_prime(512, 2512)
P1024B = recorded_prime(1024, 3024)
P2048 = recorded_prime(2048, 4048)


def mk(p, S, seed, specs, klen=32, cklen=None, vmax=None):
    """[(p, S, Item), ...] from (state_chunks, chunks), test_gpu_cxx_verify_many's items."""
    return [(p, S, it) for it in make(p, S, seed, specs, klen, cklen, vmax)]


def cm_verify(nat, items, flags=0, edit=None, fill=0xA5, fn="hb_cxx_verify_rhs_mixed"):
    """hb_cxx_verify_rhs_mixed over (p, S, Item): (rc, [rhs bytes per item], launches)."""
    ctx = nat.context()
    n = len(items)
    offs, total = [], 0
    for p, _, _ in items:
        offs.append(total)
        total += nat.width_of(p)
    out = np.full(max(total, 1), fill, dtype=np.uint8)
    descs = (nat.VerifyMixedDesc * max(n, 1))()
    keep = []
    for i, (p, S, it) in enumerate(items):
        d = descs[i]
        pb, vb, mub = nat.be(p), _be(it.vmax), _mub(p, it)
        keep.append((pb, vb, mub))
        d.p_be, d.p_len, d.sectors, d.key_len, d.chal_key_len = pb, len(pb), S, len(it.fk), len(it.ck)
        d.f_key, d.alpha_key, d.chal_key = it.fk, it.ak, it.ck
        d.state_chunks, d.chunks = it.nstate, it.chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.mu = mub
        d.rhs_out = out.ctypes.data + offs[i]
    if edit is not None:
        edit(descs)
    with ctx.lock:
        rc = getattr(nat.lib(), fn)(ctx.h, descs, n, flags)
    ln = launches(nat) if rc == 0 else None
    raw = out.tobytes()
    return rc, [raw[o:o + nat.width_of(p)] for (p, _, _), o in zip(items, offs)], ln


def check_mixed(nat, oracle, items, use_oracle=True, **kw):
    """The mixed call == hb_cxx_verify_rhs per proof == the restatement, every
    item: (results, the call's launches, the single calls' launches per item)."""
    rc, got, ln = cm_verify(nat, items, **kw)
    assert rc == 0, last_error(nat)
    singles = []
    for i, (p, S, it) in enumerate(items):
        where = (i, p.bit_length(), S, it.nstate, it.chunks)
        rc1, one = verify_single(nat, p, S, it)
        singles.append(launches(nat))
        assert rc1 == 0, last_error(nat)
        assert got[i] == one, where
        if use_oracle:
            assert got[i] == restate(oracle, p, S, it), where
    return got, ln, singles


def untouched(got):
    return all(set(g) <= {0xA5} for g in got)


def _alternate(groups):
    out = []
    for k in range(max(len(g) for g in groups)):
        out += [g[k] for g in groups if k < len(g)]
    return out


# ------------------------------------------------------------------ 0: one prime
def test_one_prime_equals_cxx_verify_rhs_many(nat, oracle):
    specs = [(1, 1), (1, 6), (4, 3), (10, 7), (10, 2 ** 32 - 1), (21, 6), (5, 0), (0, 0)]
    items = mk(P256, 3, 1, specs)
    got, ln, _ = check_mixed(nat, oracle, items)
    assert ln == 2
    rc, many = verify_many(nat, P256, 3, [it for _, _, it in items])
    assert rc == 0 and many == got and launches(nat) == 2


# ------------------------------------------------------------------ 1: alpha slots
@pytest.mark.parametrize("pa,pb", [(P128, P256), (P384, P512)], ids=["nl8", "nl16"])
def test_alpha_slots_of_neighbours(nat, oracle, pa, pb):
    """S = 1 next to 16 (and 3, 10) under alternating primes of one limb class:
    alpha and mu of proof f at its own first slot; three item orders."""
    sectors = [1, 16, 3, 10, 1, 16]
    items = []
    for k in range(12):
        p, S = (pa, pb)[k % 2], sectors[k % 6]
        nstate = [1, 7, 40][k % 3]
        items += mk(p, S, 300 + k, [(nstate, [nstate + 3, 5, 33, 1, 0][k % 5])])
    for (p0, s0, _), (p1, s1, _) in zip(items, items[1:]):
        assert p0 != p1 and s0 != s1
    got, ln, _ = check_mixed(nat, oracle, items)
    assert ln == 2                                        # one class, one group
    order = list(range(len(items)))
    random.Random(31).shuffle(order)
    for perm in (list(reversed(range(len(items)))), order):
        rc, again, ln = cm_verify(nat, [items[k] for k in perm])
        assert rc == 0 and ln == 2
        assert again == [got[k] for k in perm]


def test_every_class_and_key_length_in_one_call(nat, oracle):
    S = 3
    items = []
    for p in (P128, P256B, P384, P512, P1024B, P2048):
        for klen in (16, 24, 32):
            items += mk(p, S, p.bit_length() + klen, [(5, 3), (1, 1), (7, 9)], klen=klen)
    through = []
    for bits, seed in ((61, 2061), (257, 2257), (1000, 3000)):   # ByteCount 8, 33 and 125
        for klen in (16, 24, 32):
            through += mk(recorded_prime(bits, seed), S, bits + klen, [(5, 3)], klen=klen)
    batch = items[:20] + through[:4] + items[20:] + through[4:]
    got, ln, singles = check_mixed(nat, oracle, batch)
    fall = [s for (p, _, _), s in zip(batch, singles) if p.bit_length() in (61, 257, 1000)]
    assert len(fall) == 9 and ln == 24 + sum(fall)       # 12 classes of one group, and the single calls
    rc, alone, ln = cm_verify(nat, items)
    assert rc == 0 and ln == 24


# ------------------------------------------------------------------ 2: chunk counts, state_chunks
def test_chunk_counts_and_check_all_boundary(nat, oracle):
    counts = (0, 1, J - 1, J, J + 1, 4 * J + 1)
    a = mk(P128, 2, 41, [(4 * J + 40, n) for n in counts])                  # sampled
    b = mk(P256, 3, 42, [(n, n) for n in counts if n])                      # check_all
    a2 = mk(P128, 5, 43, [(n, n + 5) for n in counts if n])
    b2 = mk(P256B, 1, 44, [(300, n) for n in (299, 300, 305, 2 ** 32 - 1)])
    for _, _, it in b2[1:]:
        it.fk, it.ak, it.ck, it.mu = b2[0][2].fk, b2[0][2].ak, b2[0][2].ck, b2[0][2].mu
    items = _alternate([a, b]) + _alternate([b2, a2])
    got, ln, _ = check_mixed(nat, oracle, items)
    assert ln == 2
    gb = [g for (p, _, _), g in zip(items, got) if p == P256B]
    assert gb[1] == gb[2] == gb[3] != gb[0]


def test_state_chunks_widths(nat, oracle):
    """ByteCount(state_chunks) 1 to 4, neighbours under other primes."""
    sizes = (1, 255, 256, 257, 65535, 65536, 1 << 24)
    a = mk(P128, 1, 51, [(n, min(40, n - 1)) for n in sizes])
    b = mk(P256, 2, 52, [(n, min(33, n - 1) + 1) for n in sizes])
    got, ln, _ = check_mixed(nat, oracle, _alternate([a, b]))
    assert ln == 2


def test_v_max(nat, oracle):
    S = 2
    cases = [(P256, P256), (P1024B, (1 << 127) + 45), (P256B, (1 << 256) - 189), (P128, (1 << 127) + 45)]
    items = []
    for k, (p, vm) in enumerate(cases):
        items += mk(p, S, 60 + k, [(100, 30), (10, 10)], vmax=vm)
    got, ln, _ = check_mixed(nat, oracle, items)
    assert ln == 4                                        # NL 8 and NL 32
    short = mk(P256, S, 66, [(100, 30)], vmax=(1 << 39) + 7)         # 5 bytes: the single call
    got2, ln2, singles = check_mixed(nat, oracle, items[:3] + short + items[3:])
    assert got2[:3] + got2[4:] == got and ln2 == 4 + singles[3]
    wide = (1 << 256) + 1
    ok512, bad256 = mk(P512, S, 67, [(9, 5)], vmax=wide), mk(P256B, S, 68, [(9, 5)], vmax=wide)
    assert verify_single(nat, P256B, S, bad256[0][2])[0] == nat.HB_EUNSUPPORTED
    rc, out, _ = cm_verify(nat, items[:2] + ok512 + bad256 + items[2:])
    assert rc == nat.HB_EUNSUPPORTED and "proof 3: " in last_error(nat) and untouched(out)
    got3, _, _ = check_mixed(nat, oracle, items[:2] + ok512 + items[2:])
    assert got3[:2] + got3[3:] == got


# ------------------------------------------------------------------ 3: round counts, caps
def test_mixed_round_counts_fall_through(nat, oracle):
    """key_len 32 with chal_key_len 16: that proof goes through the single
    call; 24 with 24 beside it is another class's group."""
    odd = mk(P256, 2, 71, [(10, 7), (300, 70)], klen=32, cklen=16)
    same = mk(P128, 3, 72, [(10, 7), (5, 0)], klen=32) + mk(P256B, 1, 73, [(10, 10)], klen=24, cklen=24)
    items = [same[0], odd[0], same[1], same[2], odd[1]]
    got, ln, singles = check_mixed(nat, oracle, items)
    assert ln == 2 + 2 + singles[1] + singles[4]


def test_group_splitting_and_fall_through(nat, oracle, monkeypatch):
    a = mk(P128, 2, 81, [(100, 10), (10, 10), (100, 10)])
    b = mk(P256, 3, 82, [(100, 10), (10, 11), (100, 10)])
    big = mk(P256B, 1, 83, [(100, 50)])
    items = _alternate([a, b])
    items = items[:2] + big + items[2:]
    want, ln, singles = check_mixed(nat, oracle, items)
    assert ln == 2
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "20")
    try:
        rc, got, n = cm_verify(nat, items)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0 and got == want
    assert n == 3 * 2 + singles[2]
    rc, got, n = cm_verify(nat, items)
    assert rc == 0 and got == want and n == 2


# ------------------------------------------------------------------ 4: errors, the context afterwards
def test_errors_then_a_valid_batch(nat, oracle):
    items = mk(P256, 4, 91, [(100, 10)]) + mk(P128, 2, 92, [(13, 5)]) + mk(P1024B, 3, 93, [(9, 0)]) + \
        mk(P256B, 2, 94, [(1, 1)])
    want, _, _ = check_mixed(nat, oracle, items)

    def valid():
        rc, got, _ = cm_verify(nat, items)
        assert rc == 0 and got == want

    rc, got, _ = cm_verify(nat, [])
    assert rc == 0 and got == []
    for flags in (1, 2, nat.HB_PRF_CXX, nat.HB_ASYNC, 1 << 20):
        rc, got, _ = cm_verify(nat, items, flags=flags)
        assert rc == nat.HB_EUNSUPPORTED and untouched(got), flags
    valid()
    rc, got, _ = cm_verify(nat, items, flags=nat.HB_PRF_CXX, fn="hb_verify_rhs_mixed")
    assert rc == nat.HB_EUNSUPPORTED and untouched(got)
    p2049 = (1 << 2048) | 1
    pb2049, pb7 = nat.be(p2049), nat.be(0x7f)
    wider = b"\x01" + b"\0" * 32

    def spoil(**fields):
        def edit(descs):
            for k, v in fields.items():
                setattr(descs[1], k, v)
        return edit

    it1 = items[1][2]
    cases = [(spoil(p_be=pb2049, p_len=len(pb2049)), verify_single(nat, p2049, 2, it1)[0]),
             (spoil(p_be=pb7, p_len=1), verify_single(nat, 0x7f, 2, make(0x7f, 2, 95, [(13, 5)])[0])[0]),
             (spoil(p_len=0), HB_EINVAL),
             (spoil(p_be=None), HB_EINVAL),
             (spoil(sectors=0), verify_single(nat, P128, 0, it1)[0]),
             (spoil(sectors=1 << 32), HB_EINVAL),
             (spoil(key_len=15), HB_EINVAL),
             (spoil(chal_key_len=33), HB_EINVAL),
             (spoil(state_chunks=0), HB_EINVAL),
             (spoil(state_chunks=1 << 32), nat.HB_EUNSUPPORTED),
             (spoil(vmax_len=0), HB_EINVAL),
             (spoil(vmax_be=b"\0\0", vmax_len=2), HB_EINVAL),
             (spoil(vmax_be=wider, vmax_len=len(wider)), nat.HB_EUNSUPPORTED)]
    cases += [(spoil(**{f: None}), HB_EINVAL) for f in ("f_key", "alpha_key", "chal_key", "mu", "rhs_out", "vmax_be")]
    assert cases[0][1] == nat.HB_EUNSUPPORTED and cases[1][1] == HB_EINVAL and cases[4][1] == HB_EINVAL
    for edit, code in cases:
        rc, got, _ = cm_verify(nat, items, edit=edit)
        assert rc == code and "proof 1: " in last_error(nat), last_error(nat)
        assert untouched(got)
        valid()
    rc, got, _ = cm_verify(nat, items, edit=spoil(state_chunks=0))
    assert "proof 1: state has no chunks" in last_error(nat)
    ctx = nat.context()
    with ctx.lock:
        assert nat.lib().hb_cxx_verify_rhs_mixed(ctx.h, None, 3, 0) == HB_EINVAL
    valid()


def test_context_afterwards(nat, oracle, pys, swz, monkeypatch):
    items = mk(P128, 2, 101, [(30, 5), (4, 9)]) + mk(P256, 3, 102, [(300, J + 1)]) + mk(P1024B, 2, 103, [(9, 3)])
    want, _, _ = check_mixed(nat, oracle, items)
    flat = [(p, S, it.fk, it.ak, it.nstate, it.ck, it.chunks, it.vmax, it.mu) for p, S, it in items]

    def others():
        out = other_calls(nat, pys, swz, monkeypatch)
        rc, got, _ = py_verify_mixed(nat, flat)
        assert rc == 0
        out.append(got)
        rc, got = verify_many(nat, P256, 3, [items[2][2], items[2][2]])
        assert rc == 0 and got == [want[2]] * 2
        return out

    before = others()
    rc, got, _ = cm_verify(nat, items)
    assert rc == 0 and got == want
    assert others() == before
    rc, got, _ = cm_verify(nat, items)
    assert rc == 0 and got == want
    assert verify_single(nat, P256, 3, items[2][2]) == (0, want[2])


# ------------------------------------------------------------------ 5: end to end
def test_heartbeat_prove_mixed_verify_mixed(nat, swz, tmp_path):
    """Three Heartbeat beats with different primes and sector counts:
    encode -> gen_challenge -> prove_mixed -> verify_mixed at check_fraction
    1.0 and 0.3 equal the loops of prove() and verify(); honest proofs are
    accepted, one flipped file byte is rejected, a state under the wrong beat
    gives False."""
    import heartbeat
    assert heartbeat.Heartbeat is swz.Swizzle
    assert heartbeat.Heartbeat.prove_mixed is swz.Swizzle.prove_mixed
    rng = np.random.default_rng(130)
    beats = [heartbeat.Heartbeat(sectors=10, prime=P1024B), heartbeat.Heartbeat(sectors=3, prime=P256B),
             heartbeat.Heartbeat(sectors=16, prime=P512)]
    datas = [[rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (0, 777, 20000)] for _ in beats]
    encs = [b.encode_many([io.BytesIO(x) for x in ds]) for b, ds in zip(beats, datas)]
    path = tmp_path / "f.bin"
    path.write_bytes(datas[1][2])
    for fraction in (1.0, 0.3):
        items, vitems, opened = [], [], []
        for k in range(3):                                # beats interleaved
            for b, beat in enumerate(beats):
                beat.check_fraction = fraction
                tag, state = encs[b][k]
                f = io.BytesIO(datas[b][k])
                if (k, b) == (2, 1):
                    f = open(str(path), "rb")
                    opened.append(f)
                    f.seek(3)
                elif (k, b) == (1, 2):
                    f.seek(7)
                chal = beat.gen_challenge(state)
                items.append((beat.get_public(), f, chal, tag))
                vitems.append((beat, chal, state))
        try:
            want = [b.prove(f, c, t) for b, f, c, t in items]
            got = swz.Swizzle.prove_mixed(items)
            assert [(g.mu, g.sigma) for g in got] == [(x.mu, x.sigma) for x in want], fraction
            assert opened[0].tell() == 3 and items[5][1].tell() == 7     # positions restored
        finally:
            for f in opened:
                f.close()
        vit = [(beat, g, chal, state) for (beat, chal, state), g in zip(vitems, got)]
        assert heartbeat.Heartbeat.verify_mixed(vit) == [b.verify(q, c, s) for b, q, c, s in vit] == [True] * 9, fraction
    # one flipped file byte; a wrong type; a short mu; a state under the wrong beat
    bad = bytearray(datas[0][2])
    bad[len(bad) // 2] ^= 1
    for beat in beats:
        beat.check_fraction = 1.0
    chals = [b.gen_challenge(s) for b, _, s in vitems]
    fresh = [io.BytesIO(bytes(bad) if i == 6 else datas[i % 3][i // 3]) for i in range(9)]   # item 6: beat 0, file 2
    tampered = [(pub, f, c, tag) for (pub, _, _, tag), f, c in zip(items, fresh, chals)]
    got = swz.Swizzle.prove_mixed(tampered)
    vit = [(beat, g, c, state) for (beat, _, state), g, c in zip(vitems, got, chals)]
    vit.insert(2, (beats[0], got[0], "not a challenge", vitems[0][2]))           # None
    short = swz.Proof()
    short.mu, short.sigma = got[1].mu[:-1], got[1].sigma
    vit.append((beats[1], short, chals[1], vitems[1][2]))                        # len(mu) != S: False
    vit.append((beats[2], got[1], chals[1], vitems[1][2]))                       # beat 1's state under beat 2's keys: False
    want = [True, True, None, True, True, True, True, False, True, True, False, False]
    assert swz.Swizzle.verify_mixed(vit) == want == [b.verify(q, c, s) for b, q, c, s in vit]
    assert swz.Swizzle.prove_mixed([]) == [] and swz.Swizzle.verify_mixed([]) == []
    empty = swz.Tag()
    with pytest.raises(swz.HeartbeatError) as e:
        swz.Swizzle.prove_mixed([items[0], (items[1][0], io.BytesIO(b"x"), items[1][2], empty)])
    assert str(e.value) == "tag is empty"
