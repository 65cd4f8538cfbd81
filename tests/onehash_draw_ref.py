"""What the OneHash device draw must give, for its three test files: Python's
own ``random`` at test time (``expected``), the issue's rule restated in plain
Python (``key_of``, ``Generator``: the fake native's draw), and the matrix of
ranges, seeds and counts."""
import hashlib
import random

MAX_KEY_WORDS = 1024
LENS = [1, 2, 3, 1000, 1 << 20, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1, (1 << 63) + 5, (1 << 64) - 1]
SEEDS = [b"", b"root", "root", bytearray(range(100)), 0, -5, 7, (1 << 70) + 3, True, hashlib.sha256(b"digest").digest()]
NUMS = [0, 1, 5, 700, 1300]   # 700 and 1300 cross one and two regenerations
# (len, num, seed): exactly 624 words consumed -- the state is the first array with index 624
LAZY = ((1 << 40) - 1, 312, b"root")


def matrix():
    return [(length, num, seed) for length in LENS for seed in SEEDS for num in NUMS]


def expected(seed, length, num):
    """(blocks, the 625 state words) by the module-level generator itself."""
    random.seed(seed)
    blocks = [random.randint(0, length - 1) for _ in range(num)]
    version, words, gauss = random.getstate()
    assert version == 3 and gauss is None and len(words) == 625
    return blocks, list(words)


def key_of(seed):
    """The generator's key words, least significant first."""
    if isinstance(seed, (str, bytes, bytearray)):
        a = seed.encode() if isinstance(seed, str) else bytes(seed)
        n = int.from_bytes(a + hashlib.sha512(a).digest(), "big")
    else:
        n = abs(int(seed))
    words = []
    while n:
        words.append(n & 0xffffffff)
        n >>= 32
    return words or [0]


M32 = 0xffffffff


class Generator(object):
    """MT19937 as the issue states it: seeding by key, a lazy twist, and
    randint(0, length - 1) by rejection."""

    def __init__(self, key):
        mt = [19650218]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & M32)
        i, j = 1, 0
        for _ in range(max(624, len(key))):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525)) + key[j] + j) & M32
            i, j = i + 1, (j + 1) % len(key)
            if i == 624:
                mt[0], i = mt[623], 1
        for _ in range(623):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941)) - i) & M32
            i += 1
            if i == 624:
                mt[0], i = mt[623], 1
        mt[0] = 0x80000000
        self.mt, self.index = mt, 624

    def word(self):
        mt = self.mt
        if self.index == 624:
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7fffffff)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
            self.index = 0
        y = mt[self.index]
        self.index += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        return y ^ (y >> 18)

    def below(self, length):
        k = length.bit_length()
        while True:
            if k <= 32:
                r = self.word() >> (32 - k)
            else:
                lo = self.word()
                r = ((self.word() >> (64 - k)) << 32) | lo
            if r < length:
                return r

    def state(self):
        return self.mt + [self.index]


def restated(seed, length, num):
    g = Generator(key_of(seed))
    return [g.below(length) for _ in range(num)], g.state()


# ---------------------------------------------------------------- mixed batches of generate_challenges_many
# (file size, num, root seed): items whose positions the device draws, items
# that stay with pick_blocks (a float seed), and items the reference fails on
GEN_DEV = [(1000, 5, b"a"), (5000, 0, "s"), (20000, 700, 7), (20000, 4, bytearray(b"ba"))]
GEN_HOST = [(1000, 3, 2.5), (5000, 2, -0.125)]
GEN_BATCHES = [[GEN_DEV[0], GEN_HOST[0], GEN_DEV[1], GEN_DEV[2], GEN_HOST[1], GEN_DEV[3]],   # a device draw decides the state
               [GEN_DEV[3], GEN_HOST[1], GEN_DEV[2], GEN_DEV[0], GEN_HOST[0]],               # a host draw does
               [GEN_HOST[0], GEN_DEV[0], GEN_HOST[0]]]                                       # the same host draw before and after
GEN_FAILS = [(1000, 2, "no secret"),   # HeartbeatError before pick_blocks (the object has no secret)
             (0, 2, b"r")]             # ValueError inside pick_blocks, after random.seed
GEN_SIZES = (0, 1000, 5000, 20000)


def with_failure(batch, bad, where):
    at = {"front": 0, "middle": len(batch) // 2, "end": len(batch)}[where]
    return batch[:at] + [bad] + batch[at:]


def write_sized_files(directory):
    """A file of every size the batches name: {size: path}."""
    out = {}
    for size in GEN_SIZES:
        p = directory / ("f%d.bin" % size)
        p.write_bytes(hashlib.shake_128(b"file%d" % size).digest(size))
        out[size] = str(p)
    return out
