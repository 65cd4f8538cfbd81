"""GPU parity of the mixed-owner batched verify (hb_verify_rhs_mixed): the
right-hand sides of many proofs that each name their own prime, sector count
and key lengths, in two launches per group of a (limb count, AES round count)
class (hb_mixed.hpp; hb_runtime.cpp verify_mixed_impl).

Every comparison is byte for byte, every item of every batch: the mixed call
against hb_verify_rhs per proof; in addition the CPU oracle's verify accepts
that right-hand side as sigma and rejects it with one bit flipped.  Over one
prime (== hb_verify_rhs_many), neighbours that differ in modulus and S inside
one group in three orders, every limb class and key size in one call, v_max
values that are not below p next to small ones and one too wide for its own
prime only, more wave-jobs than the chip has wave positions, alpha slot
placement, group splitting and fall-through, errors.

Reference: an auditor's loop over PySwizzle.py:372-395 for many owners."""
import random

import numpy as np
import pytest

from test_gpu_parity import P256
from test_gpu_prove_many import P255, P256MAX
from test_gpu_prove_mixed import recorded_prime
from test_gpu_verify_many import _item, _mub, last_error, oracle_checks, verify_many, verify_single

pytestmark = pytest.mark.gpu

HB_EINVAL = -1


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


def mitem(rng, p, S, nstate, chunks, vmax=None, klen=32, cklen=None):
    """(p, S) + test_gpu_verify_many's item (f_key, alpha_key, state_chunks,
    chal_key, chunks, v_max, mu ints)."""
    return (p, S) + _item(rng, p, S, nstate, chunks, vmax=vmax, klen=klen, cklen=cklen)


def verify_mixed(nat, items, flags=0, edit=None, fill=0xA5):
    """hb_verify_rhs_mixed: (rc, [rhs bytes per proof], launches)."""
    ctx = nat.context()
    n = len(items)
    descs = (nat.VerifyMixedDesc * max(n, 1))()
    offs, total = [], 0
    for it in items:
        offs.append(total)
        total += nat.width_of(it[0])
    out = np.full(max(total, 1), fill, dtype=np.uint8)
    keep = []
    for i, (p, S, fk, ak, nstate, ck, chunks, vmax, mu) in enumerate(items):
        pb, vb, mb = nat.be(p), nat.be(vmax), _mub(p, mu, nat.width_of(p))
        keep.append((pb, vb, mb))
        d = descs[i]
        d.p_be, d.p_len, d.sectors, d.key_len, d.chal_key_len = pb, len(pb), S, len(fk), len(ck)
        d.f_key, d.alpha_key, d.chal_key = fk, ak, ck
        d.state_chunks, d.chunks = nstate, chunks
        d.vmax_be, d.vmax_len = vb, len(vb)
        d.mu = mb
        d.rhs_out = out.ctypes.data + offs[i]
    if edit:
        edit(descs)
    with ctx.lock:
        rc = nat.lib().hb_verify_rhs_mixed(ctx.h, descs, n, flags)
    launches = ctx.last_kernel_ms()[1] if rc == 0 else None
    raw = out.tobytes()
    return rc, [raw[o:o + nat.width_of(it[0])] for it, o in zip(items, offs)], launches


def untouched(out):
    return all(set(o) == {0xA5} for o in out)


def check_mixed(nat, oracle, items, **kw):
    """The mixed call == hb_verify_rhs per proof, and the oracle's verify agrees; every item."""
    rc, got, launches = verify_mixed(nat, items, **kw)
    assert rc == 0, last_error(nat)
    for i, it in enumerate(items):
        rc1, one = verify_single(nat, it[0], it[1], it[2:])
        assert rc1 == 0, last_error(nat)
        assert got[i] == one, (i, it[0].bit_length(), it[1], it[4], it[6])
        oracle_checks(oracle, it[0], it[1], it[2:], one)
    return got, launches


# ------------------------------------------------------------------ one prime
def test_one_prime_equals_verify_many(nat, oracle):
    S = 10
    rng = np.random.default_rng(41)
    items = [mitem(rng, P256, S, ns, n) for n in (0, 1, 16, 17, 33, 257) for ns in (1, 2, 820, (1 << 27) + 1, (1 << 40) + 3)]
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 2
    rc, many = verify_many(nat, P256, S, [it[2:] for it in items])
    assert rc == 0 and many == got


# ------------------------------------------------------------------ neighbours that differ
_neigh = {}


def neighbours(nat, oracle):
    if not _neigh:
        rng = np.random.default_rng(52)
        primes, sectors, chunks = [P256, P256MAX, P255], [1, 3, 10], [1, 15, 16, 17, 33, 257]
        items = [mitem(rng, primes[i % 3], sectors[(i + i // 3) % 3], [1, 820, (1 << 33) + 5][(i // 2) % 3],
                       chunks[(i + i // 6) % 6]) for i in range(36)]
        for a, b in zip(items, items[1:]):
            assert a[0] != b[0] and a[1] != b[1]
        got, launches = check_mixed(nat, oracle, items)
        _neigh["v"] = (items, got, launches)
    return _neigh["v"]


def test_neighbours_that_differ(nat, oracle):
    items, got, launches = neighbours(nat, oracle)
    assert launches == 2                                          # one class, one group
    order = list(range(36))
    random.Random(53).shuffle(order)
    for perm in (list(reversed(range(36))), order):
        rc, again, launches = verify_mixed(nat, [items[k] for k in perm])
        assert rc == 0 and launches == 2
        assert again == [got[k] for k in perm]


# ------------------------------------------------------------------ every class and key size in one call
def test_every_class_and_key_size_in_one_call(nat, oracle):
    S = 3
    items = []
    for bits in (20, 61, 129, 256, 257, 512, 1000, 1024, 1025, 2048):
        p = recorded_prime(bits, 2000 + bits)
        for klen in (16, 24, 32):
            rng = np.random.default_rng(bits + klen + 1)
            items += [mitem(rng, p, S, ns, n, klen=klen) for n, ns in [(1, 1), (17, 3000), (33, 1 << 33)]]
    assert len(items) == 90
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 24                                         # 4 limb classes x 3 round counts, 2 launches each
    # state and challenge keys with different round counts: the single verify, inside the same call
    rng = np.random.default_rng(7)
    odd = mitem(rng, P255, 4, 50, 20, klen=16, cklen=32)
    got2, launches = check_mixed(nat, oracle, items[:5] + [odd] + items[5:])
    # (the unfused single verify counts no launch of its own, as after hb_verify_rhs)
    assert got2[:5] + got2[6:] == got and launches >= 24


# ------------------------------------------------------------------ factors not below p
def test_vmax_not_below_p_next_to_small_ones(nat, oracle):
    S = 3
    rng = np.random.default_rng(81)
    big = [mitem(rng, P256MAX, S, 820, n, vmax=(1 << 256) - 1) for n in (1, 37, 300)]
    small = [mitem(rng, P255, S, 820, n, vmax=2) for n in (1, 37, 300)]
    items = [x for pair in zip(big, small) for x in pair]
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 2
    p512 = recorded_prime(512, 2512)
    wide = (1 << 256) + 1
    ok512 = mitem(rng, p512, S, 820, 5, vmax=wide)
    bad256 = mitem(rng, P255, S, 820, 5, vmax=wide)
    assert verify_single(nat, P255, S, bad256[2:])[0] == nat.HB_EUNSUPPORTED
    rc, out, _ = verify_mixed(nat, items[:3] + [ok512, bad256] + items[3:])
    assert rc == nat.HB_EUNSUPPORTED and "proof 4" in last_error(nat)
    assert untouched(out)
    got2, _ = check_mixed(nat, oracle, items[:3] + [ok512] + items[3:])
    assert got2[:3] + got2[4:] == got


# ------------------------------------------------------------------ more wave-jobs than wave positions
def test_more_wave_jobs_than_wave_positions(nat, oracle):
    """300 proofs x 257 chunks under alternating primes and S: 10,500 wave-jobs
    through the one new PRF instantiation."""
    rng = np.random.default_rng(54)
    items = [mitem(rng, P255 if i % 2 else P256, 10 if i % 2 else 1, 7 + i, 257) for i in range(300)]
    assert sum((it[1] + 15) // 16 + 2 * ((it[6] + 15) // 16) for it in items) > 10000
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 2


# ------------------------------------------------------------------ alpha slot placement
def test_alpha_slot_placement(nat, oracle):
    """S = 1, 40, 1 in sequence: a wrong alpha base overwrites a neighbour."""
    rng = np.random.default_rng(55)
    items = [mitem(rng, p, S, 820, n) for p, S, n in [(P256, 1, 17), (P255, 40, 33), (P256MAX, 1, 16), (P256, 40, 1),
                                                      (P255, 1, 0), (P256MAX, 17, 5)]]
    got, launches = check_mixed(nat, oracle, items)
    assert launches == 2


# ------------------------------------------------------------------ splitting, fall-through
def test_group_splitting_and_long_challenges(nat, oracle, monkeypatch):
    items, want, _ = neighbours(nat, oracle)
    rng = np.random.default_rng(112)
    p1024 = recorded_prime(1024, 3024)
    longs = [mitem(rng, P255, 3, 900, 1000), mitem(rng, p1024, 2, 900, 1000)]
    lwant, _ = check_mixed(nat, oracle, longs)
    batch = items[:20] + [longs[0]] + items[20:] + [longs[1]]
    assert sum(it[6] for it in items) > 4 * 300
    monkeypatch.setenv("HB_TEST_BATCH_CHUNKS", "300")
    try:
        rc, got, launches = verify_mixed(nat, batch)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_CHUNKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want[:20] + [lwant[0]] + want[20:] + [lwant[1]]  # the bytes do not change
    assert launches >= 2 * 5                                      # several groups (a fused single verify adds one)
    rc, got, launches = verify_mixed(nat, batch)
    assert rc == 0 and launches == 4 and got == want[:20] + [lwant[0]] + want[20:] + [lwant[1]]


# ------------------------------------------------------------------ errors, no-ops
def test_errors_and_noops(nat, oracle):
    rng = np.random.default_rng(121)
    items = [mitem(rng, P256, 4, 50, 3), mitem(rng, P255, 2, 50, 20), mitem(rng, P256MAX, 3, 50, 0)]
    want, _ = check_mixed(nat, oracle, items)

    def valid():
        rc, got, _ = verify_mixed(nat, items)
        assert rc == 0 and got == want

    rc, got, _ = verify_mixed(nat, [])
    assert rc == 0 and got == []
    for flags in (1, 2, nat.HB_PRF_CXX, 1 << 20):
        rc, got, _ = verify_mixed(nat, items, flags=flags)
        assert rc == nat.HB_EUNSUPPORTED and untouched(got)
    valid()
    p2049 = (1 << 2048) | 1
    pb2049, pb7 = nat.be(p2049), nat.be(0x7f)

    def spoil(**fields):
        def edit(descs):
            for k, v in fields.items():
                setattr(descs[1], k, v)
        return edit

    it1 = items[1]
    cases = [(spoil(p_be=pb2049, p_len=len(pb2049)), verify_single(nat, p2049, 2, it1[2:])[0]),
             (spoil(p_be=pb7, p_len=1), verify_single(nat, 0x7f, 2, it1[2:])[0]),
             (spoil(p_len=0), HB_EINVAL),
             (spoil(p_be=None), HB_EINVAL),
             (spoil(sectors=0), verify_single(nat, P255, 0, it1[2:])[0]),
             (spoil(key_len=15), HB_EINVAL),
             (spoil(chal_key_len=17), HB_EINVAL),
             (spoil(state_chunks=0), verify_single(nat, P255, 2, it1[2:4] + (0,) + it1[5:])[0]),
             (spoil(vmax_len=0), HB_EINVAL)]                       # v_max == 0 with chunks > 0
    cases += [(spoil(**{f: None}), HB_EINVAL) for f in ("f_key", "alpha_key", "chal_key", "vmax_be", "mu", "rhs_out")]
    assert cases[0][1] == nat.HB_EUNSUPPORTED and cases[1][1] == HB_EINVAL and cases[4][1] == HB_EINVAL
    assert cases[7][1] == HB_EINVAL
    for edit, code in cases:
        rc, got, _ = verify_mixed(nat, items, edit=edit)
        assert rc == code and "proof 1" in last_error(nat), last_error(nat)
        assert untouched(got)
    valid()
    ctx = nat.context()
    with ctx.lock:
        assert nat.lib().hb_verify_rhs_mixed(ctx.h, None, 3, 0) == HB_EINVAL
    valid()
