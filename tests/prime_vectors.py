"""Python references and the shared vector set of the prime tests
(test_prime_emul.py, test_gpu_mr_test.py, test_gpu_prime_search.py).

Nothing here comes from the code under test: sprp() is the strong probable
prime test written with pow(), search_ref() the definition of hb_prime_search
("the first k in the window with n < 2^bits that passes base 2 and the given
bases").  Its private trial division only skips candidates that have a proper
factor, so it cannot remove a prime.
"""
import functools
import hashlib
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIT_LENGTHS = (8, 31, 32, 33, 64, 65, 129, 256, 257, 512, 513, 1000, 1024, 1025, 2047, 2048)
_SMALL = [q for q in range(3, 2000, 2) if all(q % d for d in range(3, int(q ** 0.5) + 1, 2))]


def sprp(n, a):
    """Is odd n >= 5 a strong probable prime to base a, 2 <= a <= n - 2?"""
    assert n >= 5 and n & 1 and 2 <= a <= n - 2
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    x = pow(a, d, n)
    if x == 1 or x == n - 1:
        return True
    for _ in range(s - 1):
        x = x * x % n
        if x == n - 1:
            return True
    return False


def nl_of_width(width):
    bits = 8 * width
    for lim, nl in ((64, 2), (256, 8), (512, 16), (1024, 32), (2048, 64)):
        if bits <= lim:
            return nl
    raise ValueError(width)


def search_ref(bits, start, bases, window):
    """The smallest start + 2k, k < window, below 2^bits, that is a strong
    probable prime to base 2 and to every base; None if there is none."""
    for k in range(window):
        n = start + 2 * k
        if n >> bits:
            return None
        if any(n % q == 0 and n != q for q in _SMALL):
            continue
        if sprp(n, 2) and all(sprp(n, a) for a in bases):
            return n
    return None


def shake_start(bits, i):
    """SHAKE-256("hb-prime-<bits>-<i>") masked to `bits`, top and low bits set."""
    raw = hashlib.shake_256(("hb-prime-%d-%d" % (bits, i)).encode()).digest((bits + 7) // 8)
    return (int.from_bytes(raw, "big") & ((1 << bits) - 1)) | (1 << (bits - 1)) | 1


@functools.lru_cache(maxsize=None)
def recorded_primes():
    with open(os.path.join(GOLDEN, "mixed_primes.json")) as fh:
        d = json.load(fh)
    return {int(k.split("/")[0]): int(v, 16) for k, v in d.items() if k != "generator"}


@functools.lru_cache(maxsize=None)
def prime_of(bits):
    """A prime of exactly `bits` bits: the recorded one, else the first after
    a seeded start (host pow)."""
    rec = recorded_primes()
    if bits in rec:
        return rec[bits]
    start = shake_start(bits, 99)
    bases = [3, 5, 7, 11, 13]
    while True:
        n = search_ref(bits, start, [a for a in bases if a <= start - 2], 1 << 16)
        if n is not None:
            return n
        start = shake_start(bits, start & 0xffff)


def _bases(rng, n):
    out = [2, n - 2]
    for _ in range(2):
        out.append(rng.randrange(2, n - 1))
    return out


@functools.lru_cache(maxsize=None)
def vectors():
    """[(width, n, [a0, a1, a2, a3])]: width in bytes (the limb class follows
    from it), n odd >= 5, four bases in [2, n - 2]: 2, n - 2, two seeded."""
    rng = random.Random(0x5eed9)
    rec = recorded_primes()
    cands = []   # (width, n)

    def add(n, width=None):
        assert n >= 5 and n & 1
        cands.append(((n.bit_length() + 7) // 8 if width is None else width, n))

    for b in BIT_LENGTHS:
        wide = b > 1025   # NL = 64: a handful
        add(prime_of(b) if not wide or b in rec else rng.getrandbits(b) | (1 << (b - 1)) | 1)
        add(3 * (1 << (b - 2)) + 1)                       # k 2^m + 1, m = bits - 2
        if wide:
            continue
        add(rng.getrandbits(b) | (1 << (b - 1)) | 1)
        add(rng.getrandbits(b) | (1 << (b - 1)) | 1)
        add((1 << b) - 1)                                 # 2^k - 1: all-ones limbs
        add((1 << (b - 1)) + 1)                           # 2^k + 1
        add((rng.getrandbits(b // 2 - 2) | (1 << (b // 2 - 3)) | 1) * (1 << (b // 2)) + 1)   # large s
        if b > 40:
            add(((1 << b) - 1) ^ (rng.getrandbits(31) << 1))   # all-ones upper limbs, random low limb
    for n in (5, 7, 9, 561, 2047, 65537, (1 << 32) + 1, 3215031751):
        add(n)
    add(561, 8)                                           # leading zero bytes
    add(3215031751, 32)
    # squares and products of recorded primes
    add(rec[20] ** 2)
    add(rec[61] * rec[129])
    add(rec[256] ** 2)
    add(rec[512] ** 2)
    add(rec[1000] * rec[20])
    add(rec[1024] ** 2)
    # small values inside the widest class
    add(561, 256)
    add(65537, 256)
    add(rec[61], 256)
    return tuple((w, n, tuple(_bases(rng, n))) for w, n in cands)
