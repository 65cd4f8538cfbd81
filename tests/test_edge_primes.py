"""The recorded edge primes (tests/edge_primes.py) are primes, of the stated
bit length, and -- for the widths up to 256 bits -- really the largest below
2^b and the smallest above 2^(b-1): no odd number between the entry and the
power of two passes the project's Miller-Rabin test."""
import importlib

import pytest

import edge_primes as E


@pytest.fixture(scope="module")
def is_prime():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")._is_probable_prime


@pytest.mark.parametrize("b", E.BITS)
def test_edge_primes_are_primes(is_prime, b):
    hi, lo = E.pmax(b), E.pmin(b)
    assert hi.bit_length() == b and lo.bit_length() == b
    assert hi < (1 << b) and lo > (1 << (b - 1)) and lo <= hi
    assert hi & 1 and lo & 1
    assert is_prime(hi), ("max", b)
    assert is_prime(lo), ("min", b)
    assert E.edge(b, "max") == hi and E.edge(b, "min") == lo
    assert E.pair(b) == [("max", hi), ("min", lo)]


@pytest.mark.parametrize("b", [b for b in E.BITS if b <= 256])
def test_edge_primes_are_extremal(is_prime, b):
    for n in range(E.pmax(b) + 2, 1 << b, 2):
        assert not is_prime(n), ("a prime above max", b, (1 << b) - n)
    for n in range((1 << (b - 1)) + 1, E.pmin(b), 2):
        assert not is_prime(n), ("a prime below min", b, n - (1 << (b - 1)))


def test_every_width_has_a_limb_class():
    assert sorted(b for bits in E.NL_BITS.values() for b in bits) == list(E.BITS)
    below = {2: 0, 8: 64, 16: 256, 32: 512, 64: 1024}   # the next smaller class's bits
    for nl, bits in E.NL_BITS.items():
        for b in bits:
            assert below[nl] < b <= 32 * nl
