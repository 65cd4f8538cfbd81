"""hb_prime_search on the GPU against its definition written in Python
(tests/prime_vectors.py search_ref: the first k in the window with n < 2^bits
that passes base 2 and the given bases, by pow()): exhaustive-style sweeps at
small sizes and every window, the named edge cases (windows without a prime,
the window leaving `bits` bits, a candidate that is itself a sieve prime, a
prime start), and seeded starts at 256, 1000, 1024 and 2048 bits."""
import random

import pytest

import prime_vectors as pv

pytestmark = pytest.mark.gpu


def search(bits, starts, bases, window):
    from heartbeat_amd import primes
    stats = {}
    got = primes.prime_search(bits, starts, bases, window, stats)
    return got, stats


def bases_for(rng, bits, rounds):
    return [rng.randrange(2, 1 << (bits - 1)) for _ in range(rounds)]


@pytest.mark.parametrize("bits", [8, 9, 16, 17, 33, 64, 65, 128])
def test_small_sizes_every_window(bits):
    rng = random.Random(bits)
    top = 1 << (bits - 1)
    if bits <= 9:
        starts = list(range(top + 1, 1 << bits, 2))           # every start
    else:
        starts = [top + 1, (1 << bits) - 1, (1 << bits) - 3, (1 << bits) - 201]
        starts += [rng.getrandbits(bits) | top | 1 for _ in range(60)]
        starts += [((1 << bits) - 1) - 2 * rng.randrange(0, 3000) for _ in range(30)]   # near 2^bits
    for window in (1, 5, 64, 1024):
        for rounds in (0, 3):
            bases = [bases_for(rng, bits, rounds) for _ in starts]
            got, stats = search(bits, starts, bases, window)
            want = [pv.search_ref(bits, s, b, window) for s, b in zip(starts, bases)]
            assert got == want, (bits, window, rounds,
                                 [(s, g, w) for s, g, w in zip(starts, got, want) if g != w][:3])
            assert stats["tests"] > 0 or all(w is None for w in want)
    assert any(w is not None for w in want) and all(w is None or w >> (bits - 1) == 1 for w in want)


def test_named_cases():
    def one(bits, start, window, bases=(3, 5)):
        (got,), stats = search(bits, [start], [list(bases)], window)
        assert got == pv.search_ref(bits, start, list(bases), window), (bits, start, window)
        return got
    assert one(8, 201, 5) is None                   # 201 .. 209: no prime
    assert one(8, 253, 8) is None                   # the window leaves 8 bits
    assert one(16, 65523, 100) is None              # 65521 is the last 16-bit prime
    assert one(8, 129, 64) == 131                   # the candidate is a sieve prime itself
    assert one(8, 131, 1) == 131                    # a prime start: k = 0
    assert one(16, 65521, 1) == 65521
    assert one(16, 32771, 7) == 32771
    p = pv.prime_of(64)
    assert one(64, p, 1) == p and one(64, p - 2, 2) == p and one(64, p - 2, 1) is None
    assert one(64, p - 2 * 63, 64) == pv.search_ref(64, p - 2 * 63, [3, 5], 64)


def test_raw_outputs_found_and_zero_slots():
    """found[i] and the prime slot agree: no found[i] with a zero prime, zero
    bytes where nothing was found, tests_out counts lanes."""
    import ctypes
    from heartbeat_amd import _native, multi
    ctx = multi.primary_context()
    starts = [201, 129, 253, 131, 211]
    sb = b"".join(s.to_bytes(1, "big") for s in starts)
    bb = bytes([3, 5] * len(starts))
    primes = ctypes.create_string_buffer(b"\xee" * len(starts), len(starts))
    found = ctypes.create_string_buffer(b"\xee" * len(starts), len(starts))
    tests = ctypes.c_uint64(0)
    with ctx.lock:
        ctx.check(_native.lib().hb_prime_search(ctx.h, 8, sb, len(starts), 5, bb, 2, primes, found, ctypes.byref(tests)))
    want = [pv.search_ref(8, s, [3, 5], 5) for s in starts]
    assert want == [None, 131, None, 131, 211]
    assert list(found.raw) == [int(w is not None) for w in want]
    assert list(primes.raw) == [w or 0 for w in want]
    assert tests.value > 0
    # rejected arguments: nothing written
    for bad_starts, bad_bases, bits, window in (([200], [3, 5], 8, 5), ([127], [3, 5], 8, 5), ([129], [3, 128], 8, 5),
                                                ([129], [1, 5], 8, 5), ([129], [3, 5], 8, 0), ([129], [3, 5], 8, 65537),
                                                ([129], [3, 5], 7, 5)):
        primes = ctypes.create_string_buffer(b"\xee", 1)
        found = ctypes.create_string_buffer(b"\xee", 1)
        with ctx.lock:
            rc = _native.lib().hb_prime_search(ctx.h, bits, bytes(bad_starts), 1, window, bytes(bad_bases), 2, primes,
                                               found, None)
        assert rc == -1 and primes.raw == b"\xee" and found.raw == b"\xee", (bad_starts, bad_bases, bits, window)


@pytest.mark.parametrize("bits,count,window", [(256, 8, 1024), (1000, 4, 4096), (1024, 4, 4096), (2048, 2, 8192)])
def test_seeded_starts(bits, count, window):
    rng = random.Random(bits + 1)
    starts = [pv.shake_start(bits, i) for i in range(count)]
    rounds = 3
    bases = [bases_for(rng, bits, rounds) for _ in starts]
    want = [pv.search_ref(bits, s, b, window) for s, b in zip(starts, bases)]
    assert all(w is not None for w in want)          # seeds whose windows hold a prime
    got, stats = search(bits, starts, bases, window)
    assert got == want, [(w - s) // 2 for s, w in zip(starts, want)]
    assert stats["tests"] > 0 and stats["launches"] >= 3
    assert all(g.bit_length() == bits and g & 1 for g in got)
