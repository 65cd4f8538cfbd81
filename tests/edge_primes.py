"""Edge primes of the widths the kernels are built for: for each bit length b
the largest prime below 2^b ("max" = 2^b - off) and the smallest prime above
2^(b-1) ("min" = 2^(b-1) + off).  Under "max" a sector of 0xFF bytes is >= p
when b % 8 == 0; under "min" every sector whose top bit is set is >= p, up to
almost 2p; `half`, `kz` and `p 2^w` of the split wide MAC sit at the ends of
their ranges.  The offsets were found with Miller-Rabin on the CPU and are
checked by test_edge_primes.py with the project's _is_probable_prime.
"""

# b: (max offset below 2^b, min offset above 2^(b-1))
OFFSETS = {
    32: (5, 11),
    61: (1, 33),
    64: (59, 29),
    128: (159, 29),
    255: (19, 79),
    256: (189, 95),
    384: (317, 369),
    512: (569, 111),
    1000: (1245, 1239),
    1020: (537, 285),
    1024: (105, 1155),
    2048: (1557, 1919),
}

BITS = tuple(sorted(OFFSETS))

# limbs of the kernel instantiation a width maps to (nl_of_width in prime_vectors.py)
NL_BITS = {2: (32, 61, 64), 8: (128, 255, 256), 16: (384, 512), 32: (1000, 1020, 1024), 64: (2048,)}


def pmax(b):
    """The largest prime below 2^b."""
    return (1 << b) - OFFSETS[b][0]


def pmin(b):
    """The smallest prime above 2^(b-1) (b bits)."""
    return (1 << (b - 1)) + OFFSETS[b][1]


def edge(b, which):
    return {"max": pmax, "min": pmin}[which](b)


def pair(b):
    """[("max", p), ("min", p)] of one width."""
    return [("max", pmax(b)), ("min", pmin(b))]
