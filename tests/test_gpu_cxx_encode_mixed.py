"""GPU parity of the cxx mixed-owner encode (hb_cxx_encode_mixed,
Swizzle.encode_mixed = heartbeat.Heartbeat.encode_mixed): the tags of many
files that each name their own prime, sector count and key length, with the cxx
prf, in one call (hb_emixed.hpp; hb_runtime.cpp encode_mixed_impl).

Every comparison is byte for byte, every file of every batch: the mixed call
against hb_encode(HB_PRF_CXX) per file and against the oracle's cxx encode, and
tries_out against the sum of the single calls' tries -- the cases of
tests/test_gpu_encode_mixed.py, whose helpers these tests share, over the
primes the cxx prf takes (ByteCount a multiple of 16), plus the block that
reads no sector (a length that is a multiple of the file's OWN block size, and
the empty file) next to neighbours that read sectors, and a prime whose
ByteCount is no multiple of 16 failing the call.

Reference: a loop over cxx/shacham_waters_private.cxx:638-702 for many owners
(one prime per Swizzle, :596-624)."""
import importlib

import numpy as np
import pytest

from test_gpu_parity import P256
from test_gpu_prove_many import P255, P256MAX, last_error
from test_gpu_encode_mixed import (_bytes, boundary_lengths, check_mixed, check_rejected, device_case, encode_mixed,
                                   end_to_end, geometry, large_file_case, mfile, nblocks, oracle_raw, recorded_prime,
                                   untouched)

pytestmark = pytest.mark.gpu

HB_EINVAL = -1


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def swz():
    return importlib.import_module("heartbeat_amd.Swizzle")


# ------------------------------------------------------------------ 1: one prime, one S
def cxx_encode_many(nat, p, S, items):
    """hb_cxx_encode_many over the items' keys and bytes: (rc, [tag bytes], tries)."""
    import ctypes
    ctx = nat.context()
    n = len(items)
    descs = (nat.FileDesc * n)()
    arrs, outs = [], []
    for i, it in enumerate(items):
        a = np.frombuffer(it[4], dtype=np.uint8)
        out = np.empty(nblocks(p, S, len(it[4])) * nat.width_of(p), dtype=np.uint8)
        arrs.append(a)
        outs.append(out)
        descs[i].f_key, descs[i].alpha_key = it[2], it[3]
        descs[i].data = a.ctypes.data if len(a) else None
        descs[i].len = len(it[4])
        descs[i].tags = out.ctypes.data
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        rc = nat.lib().hb_cxx_encode_many(ctx.h, pb, len(pb), S, 32, descs, n, 0, ctypes.byref(tries))
    return rc, [o.tobytes() for o in outs], tries.value


def test_one_prime_equals_cxx_encode_many(nat, oracle):
    S = 10
    rng = np.random.default_rng(10)
    items = [mfile(rng, P256, S, ln) for ln in boundary_lengths(P256, S) + [5000, 12345]]
    got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
    assert launches == 3
    rc, many, tries1 = cxx_encode_many(nat, P256, S, items)
    assert rc == 0 and many == got and tries1 == tries


# ------------------------------------------------------------------ 2: neighbours that differ, the no-sector block
_neigh = {}


def neighbours(nat, oracle):
    """36 files, one limb class, every neighbour under another modulus,
    geometry (ss 31 / 32) and S.  Every third file's length is a multiple of
    its OWN block size (the empty file included): its last block reads no
    sector and keeps F as the prf returned it, next to neighbours whose last
    block reads one."""
    if not _neigh:
        rng = np.random.default_rng(20)
        primes, sectors = [P255, P256, P256MAX], [2, 3, 10]
        items = []
        for i in range(36):
            p, S = primes[i % 3], sectors[(i + i // 3) % 3]
            ss, C = geometry(p, S)
            items.append(mfile(rng, p, S, [0, C - 1, 3 * C, 40 * C + 1, ss + 1, C][i % 6]))
        assert len({(it[0], it[1]) for it in items}) == 9
        assert sum(len(it[4]) % geometry(it[0], it[1])[1] == 0 for it in items) == 18
        got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
        _neigh["v"] = (items, got, tries, launches)
    return _neigh["v"]


def test_neighbours_that_differ_in_three_orders(nat, oracle):
    items, got, tries, launches = neighbours(nat, oracle)
    assert launches == 3
    order = [k for pair in zip(range(18), range(35, 17, -1)) for k in pair]
    for perm in (list(reversed(range(36))), order):
        rc, again, tries2, launches = encode_mixed(nat, [items[k] for k in perm], cxx=True)
        assert rc == 0 and launches == 3
        assert again == [got[k] for k in perm]
        assert tries2 == tries


def test_group_of_no_sector_blocks_only(nat, oracle):
    """Empty files and files of exactly one block under three primes: the only
    MAC blocks are the one-block files'; with empty files alone, no MAC launch."""
    rng = np.random.default_rng(25)
    empties = [mfile(rng, p, S, 0) for p, S in ((P255, 3), (P256, 10), (P256MAX, 1), (P256, 300))]
    got, tries, launches = check_mixed(nat, oracle, empties, cxx=True)
    assert launches == 2                                          # PRF and conversion
    full = [mfile(rng, p, S, geometry(p, S)[1]) for p, S in ((P255, 3), (P256, 10))]
    # 96 bytes: one whole block of the neighbour's geometry (S = 3), a block and a half of its own (S = 2)
    other = [mfile(rng, P256, 3, 96), mfile(rng, P256, 2, 96)]
    got, tries, launches = check_mixed(nat, oracle, [empties[0], full[0], other[0], other[1], empties[1], full[1]], cxx=True)
    assert launches == 3


# ------------------------------------------------------------------ 3: S at every MAC boundary
@pytest.mark.parametrize("bits,T", [(256, 256), (1024, 256), (2048, 128)])
def test_sector_counts_at_every_mac_boundary(nat, oracle, bits, T):
    p = P256 if bits == 256 else recorded_prime(bits)
    rng = np.random.default_rng(30 + bits)
    items = []
    for S in sorted({1, 2, 3, 16, 17, T - 1, T, T + 1, 255, 256, 257}):
        ss, C = geometry(p, S)
        for ln in (0, C + ss + 1, (T // S if 2 <= S <= T else 256) * C + 1 if S <= T else 2 * C):
            items.append(mfile(rng, p, S, ln))
    got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
    assert launches == 4


# ------------------------------------------------------------------ 4: file lengths per geometry
def test_file_lengths_at_each_files_own_boundaries(nat, oracle):
    rng = np.random.default_rng(40)
    shapes = [(P256, 10), (P255, 3), (P256MAX, 16), (P256, 1)]
    per = [[mfile(rng, p, S, ln) for ln in boundary_lengths(p, S)] for p, S in shapes]
    items = [per[k][i] for i in range(max(len(x) for x in per)) for k in range(len(per)) if i < len(per[k])]
    got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
    assert launches == 4
    items = []
    for bits, S, T in ((1024, 10, 256), (2048, 4, 128), (512, 7, 256)):
        p = recorded_prime(bits)
        items += [mfile(rng, p, S, ln) for ln in boundary_lengths(p, S, T)]
    check_mixed(nat, oracle, items, cxx=True)


# ------------------------------------------------------------------ 5: every class and key size in one call
def test_every_class_and_key_size_in_one_call(nat, oracle):
    S = 3
    items = []
    for bits in (255, 256, 512, 1024, 2048):
        p = P255 if bits == 255 else recorded_prime(bits)
        ss, C = geometry(p, S)
        for klen in (16, 24, 32):
            rng = np.random.default_rng(bits + klen)
            items += [mfile(rng, p, S, ln, klen=klen) for ln in (0, 4 * C + ss // 2 + 1, C - 1, 2 * C)]
    assert len(items) == 60
    got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
    assert launches == 36                                         # 4 limb classes x 3 round counts, 3 launches each


# ------------------------------------------------------------------ 6: the recorded files under the cxx prf
def test_golden_files_in_one_call(nat, oracle, golden_encode):
    """Every recorded case whose prime the cxx prf takes (the 255-, 256- and
    1024-bit ones), keys and bytes as recorded; the oracle's cxx encode is the
    reference (the recorded tags are PySwizzle's)."""
    items = []
    for c in golden_encode["cases"]:
        p = int(c["prime"], 16)
        if nat.width_of(p) % 16 == 0:
            items.append((p, c["sectors"], bytes.fromhex(c["f_key"]), bytes.fromhex(c["alpha_key"]), bytes.fromhex(c["data"])))
    assert len(items) == 114 and {it[0].bit_length() for it in items} == {255, 256, 1024}
    check_mixed(nat, oracle, items, cxx=True, single=False)


# ------------------------------------------------------------------ 7: equal inputs, repeated primes
def test_equal_bytes_and_keys_under_different_primes(nat, oracle):
    rng = np.random.default_rng(70)
    fk, ak, data = _bytes(rng, 32), _bytes(rng, 32), _bytes(rng, 1536)
    primes = [P256, P255, P256MAX, P256, P255, P256]
    items = [(p, 4, fk, ak, data) for p in primes]
    got, tries, launches = check_mixed(nat, oracle, items, cxx=True)
    assert got[0] == got[3] == got[5] and got[1] == got[4]
    assert len(set(got)) == 3


# ------------------------------------------------------------------ 8: where the bytes live
def test_device_and_host_resident_mixes(nat, oracle):
    items, got, tries, launches = neighbours(nat, oracle)
    rng = np.random.default_rng(80)
    p1024 = recorded_prime(1024)
    wide = [mfile(rng, p1024, 10, ln) for ln in (0, 1279, 1280 * 3, 5000)]
    wgot, _, _ = check_mixed(nat, oracle, wide, cxx=True)
    device_case(nat, oracle, items[:20] + wide, got[:20] + wgot, cxx=True)


# ------------------------------------------------------------------ 9: splitting, fall-through
def test_group_splitting(nat, oracle, monkeypatch):
    items, want, tries, _ = neighbours(nat, oracle)
    blocks = [nblocks(it[0], it[1], len(it[4])) for it in items]
    cap = max(sum(blocks) // 3, max(blocks))
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", str(cap))
    try:
        rc, got, tries2, launches = encode_mixed(nat, items, cxx=True)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0, last_error(nat)
    assert got == want and tries2 == tries
    assert launches >= 9


def test_large_file_falls_through_under_its_own_prime(nat, oracle, monkeypatch):
    large_file_case(nat, oracle, monkeypatch, True)


# ------------------------------------------------------------------ 10: rejected descriptors
def test_each_rejected_descriptor(nat, oracle):
    items, _, _, _ = neighbours(nat, oracle)
    check_rejected(nat, items[:6], cxx=True)


def test_bytecount_not_a_multiple_of_16_fails_the_call(nat, oracle):
    items, _, _, _ = neighbours(nat, oracle)
    rng = np.random.default_rng(100)
    for bits in (129, 1000, 1025):
        bad = mfile(rng, recorded_prime(bits), 3, 500)
        rc, got, tries, _ = encode_mixed(nat, items[:3] + [bad] + items[3:5], cxx=True)
        assert rc == nat.HB_EUNSUPPORTED, (bits, rc)
        assert last_error(nat).startswith("file 3: "), last_error(nat)
        assert untouched(got) and tries == 0


# ------------------------------------------------------------------ 11: flags, the empty call
@pytest.mark.parametrize("flag", ["HB_PRF_CXX", "HB_ASYNC", "HB_ENCODE_SINGLE_PASS", "HB_HOST_REGISTER"])
def test_unsupported_flags(nat, oracle, flag):
    items, _, _, _ = neighbours(nat, oracle)
    rc, got, _, _ = encode_mixed(nat, items[:4], cxx=True, flags=getattr(nat, flag))
    assert rc == nat.HB_EUNSUPPORTED
    assert untouched(got)


def test_empty_call(nat):
    rc, got, tries, _ = encode_mixed(nat, [], cxx=True)
    assert rc == 0 and got == [] and tries == 0


# ------------------------------------------------------------------ 12: the context afterwards
def test_context_left_clean(nat, oracle, swz):
    import io
    items, got, _, _ = neighbours(nat, oracle)
    rc, again, _, _ = encode_mixed(nat, items[:9], cxx=True)
    assert rc == 0 and again == got[:9]
    rng = np.random.default_rng(120)
    S = 10
    many = [mfile(rng, P256, S, ln) for ln in (0, 319, 320, 2000)]
    rc, tags, _ = cxx_encode_many(nat, P256, S, many)
    assert rc == 0 and tags == [oracle_raw(oracle, it, True) for it in many]
    # a plain encode, a prove and a verify through the cxx Swizzle
    beat = swz.Swizzle(sectors=S, prime=P256)
    blob = many[3][4]
    tag, state = beat.encode(io.BytesIO(blob))
    chal = beat.gen_challenge(state)
    proof = beat.get_public().prove(io.BytesIO(blob), chal, tag)
    assert beat.verify(proof, chal, state)
    st = swz.State.fromdict(state.todict())
    st.decrypt(beat.k_enc, beat.k_mac)
    assert tag.sigma == oracle.cxx_encode(P256, S, st.f_key, st.alpha_key, blob)


# ------------------------------------------------------------------ 13: end to end
def test_encode_prove_verify_mixed_end_to_end(nat, oracle, swz):
    import heartbeat
    assert heartbeat.Heartbeat is swz.Swizzle
    beats = [heartbeat.Heartbeat(sectors=16, prime=P256), heartbeat.Heartbeat(sectors=10, prime=recorded_prime(1024)),
             heartbeat.Heartbeat(sectors=3, prime=P255)]
    end_to_end(beats, swz, np.random.default_rng(130))
