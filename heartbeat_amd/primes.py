"""Drawing primes on the GPU (hb_mr_test, hb_prime_search; csrc/hb_prime.hpp).

``getPrime`` (PySwizzle.py) draws one prime on the host: trial division, then
Miller-Rabin rounds of ``pow()``.  Every owner object draws its own, so the
many-owner batches (``prove_mixed``, ``encode_mixed`` ...) spend far longer
creating their owners than running.  Here the tests of many candidates and
many bases run as one lane each:

    mr_test(cands, bases)                    strong-probable-prime verdicts
    prime_search(bits, starts, bases, window)  the first such prime after each start
    getPrimes(bits, count)                   `count` random primes

All three need a GPU (HeartbeatError without one); ``getPrime`` and the
constructors that call it stay on the host.
"""
import ctypes
import os

from . import _native, multi
from .exc import HeartbeatError

__all__ = ["mr_test", "prime_search", "getPrimes"]


def mr_test(cands, bases):
    """[bool]: is cands[i] (odd, >= 5) a strong probable prime to EVERY base of
    bases[i] (each in [2, n - 2]; the same number of bases, at least one, for
    every candidate)?  The exact function of hb_mr_test, not "is prime":
    3215031751 with bases 2, 3, 5, 7 gives True."""
    cands = [int(n) for n in cands]
    bases = [[int(a) for a in row] for row in bases]
    if len(bases) != len(cands):
        raise HeartbeatError("one row of bases per candidate")
    rounds = len(bases[0]) if bases else 1
    if any(len(row) != rounds for row in bases):
        raise HeartbeatError("every candidate takes the same number of bases")
    if any(n < 0 for n in cands) or any(a < 0 for row in bases for a in row):
        raise HeartbeatError("candidates and bases must not be negative")
    width = max([1] + [(n.bit_length() + 7) // 8 for n in cands])
    if any(a.bit_length() > 8 * width for row in bases for a in row):
        raise HeartbeatError("a base is wider than every candidate")
    cb = b"".join(n.to_bytes(width, "big") for n in cands)
    bb = b"".join(a.to_bytes(width, "big") for row in bases for a in row)
    out = ctypes.create_string_buffer(max(1, len(cands)))
    ctx = multi.primary_context()
    with ctx.lock:
        ctx.check(_native.lib().hb_mr_test(ctx.h, cb, width, len(cands), bb, rounds, out))
    return [b != 0 for b in out.raw[:len(cands)]]


def prime_search(bits, starts, bases, window, stats=None):
    """For each start (odd, exactly `bits` bits) the smallest start + 2k,
    k < window, below 2^bits, that is a strong probable prime to base 2 and to
    every base of bases[i] (each in [2, 2^(bits-1) - 1]); None where the
    window holds none (hb_prime_search).  stats: a dict that receives
    ``tests`` (lane tests run) and ``launches``."""
    bits = int(bits)
    starts = [int(s) for s in starts]
    bases = [[int(a) for a in row] for row in bases]
    if len(bases) != len(starts):
        raise HeartbeatError("one row of bases per start")
    rounds = len(bases[0]) if bases else 0
    if any(len(row) != rounds for row in bases):
        raise HeartbeatError("every start takes the same number of bases")
    width = (bits + 7) // 8
    if bits < 1 or any(s < 0 or s.bit_length() > 8 * width for s in starts) or any(
            a < 0 or a.bit_length() > 8 * width for row in bases for a in row):
        raise HeartbeatError("starts and bases must fit `bits` bits")
    sb = b"".join(s.to_bytes(width, "big") for s in starts)
    bb = b"".join(a.to_bytes(width, "big") for row in bases for a in row)
    primes = ctypes.create_string_buffer(max(1, len(starts) * width))
    found = ctypes.create_string_buffer(max(1, len(starts)))
    tests = ctypes.c_uint64(0)
    ctx = multi.primary_context()
    with ctx.lock:
        ctx.check(_native.lib().hb_prime_search(ctx.h, bits, sb, len(starts), int(window), bb or None, rounds,
                                                primes, found, ctypes.byref(tests)))
    if stats is not None:
        stats["tests"] = stats.get("tests", 0) + tests.value
        stats["launches"] = stats.get("launches", 0) + (ctx.last_kernel_ms()[1] if starts else 0)
    raw = primes.raw
    return [int.from_bytes(raw[i * width:(i + 1) * width], "big") if found.raw[i] else None
            for i in range(len(starts))]


def getPrimes(bits, count, rounds=40, window=None, stats=None):
    """`count` random primes of exactly `bits` bits (8 <= bits <= 2048), drawn
    on the GPU: random starts with the top and the low bit set and `rounds`
    random Miller-Rabin bases each come from os.urandom, and each start's
    prime is the first strong probable prime (to base 2 and those bases) among
    the `window` odd numbers from it (default 4 * bits: a window without a
    prime has probability about e^-11); starts that found nothing are drawn
    again.  count == 0 gives [].

    Like OpenSSL's incremental search, this favours primes that follow long
    gaps: a prime is chosen with probability proportional to the distance from
    the prime before it (capped by the window), not uniformly.  ``getPrime``
    redraws every candidate and has no such bias."""
    bits, count, rounds = int(bits), int(count), int(rounds)
    if count < 0:
        raise HeartbeatError("count must not be negative")
    if bits < 8 or bits > 2048:
        raise HeartbeatError("prime size must be between 8 and 2048 bits")
    if count == 0:
        return []
    window = min(4 * bits, 65536) if window is None else int(window)
    width = (bits + 7) // 8
    top = 1 << (bits - 1)
    out = []
    while len(out) < count:
        need = count - len(out)
        starts = [(int.from_bytes(os.urandom(width), "big") & (top - 1)) | top | 1 for _ in range(need)]
        # bases uniform in [2, 2^(bits-1) - 1]
        bases = [[2 + int.from_bytes(os.urandom(width + 8), "big") % (top - 2) for _ in range(rounds)]
                 for _ in range(need)]
        out.extend(p for p in prime_search(bits, starts, bases, window, stats) if p is not None)
    return out
