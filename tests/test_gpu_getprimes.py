"""getPrimes and generate_many on the GPU: exact bit length, odd, prime by the
package's host Miller-Rabin (_is_probable_prime, independent random bases),
and the owners they make run the mixed flows end to end."""
import hashlib
import importlib
import io

import pytest

pytestmark = pytest.mark.gpu


def host_is_prime(n):
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    return pys._is_probable_prime(n)


@pytest.mark.parametrize("bits,count", [(1024, 4), (256, 16)])
def test_getprimes(bits, count):
    from heartbeat_amd.PySwizzle.PySwizzle import getPrimes
    stats = {}
    ps = getPrimes(bits, count, stats=stats)
    assert len(ps) == count and len(set(ps)) == count
    for p in ps:
        assert p.bit_length() == bits and p & 1 and host_is_prime(p)
    assert stats["tests"] > 0 and stats["launches"] > 0


def test_getprimes_small_and_empty():
    from heartbeat_amd import primes
    ps = primes.getPrimes(8, 40)                    # duplicates are allowed
    assert len(ps) == 40
    small = [q for q in range(129, 256, 2) if all(q % d for d in range(3, 16, 2))]
    assert all(p in small for p in ps)
    assert primes.getPrimes(1024, 0) == [] and primes.getPrimes(8, 0) == []
    ps = primes.getPrimes(64, 3, rounds=2, window=7)   # a short window: redraws
    assert len(ps) == 3 and all(p.bit_length() == 64 and host_is_prime(p) for p in ps)


def test_pyswizzle_generate_many_end_to_end():
    from heartbeat_amd.PySwizzle import PySwizzle
    beats = PySwizzle.generate_many(3, primebits=256)
    assert len(beats) == 3 and len({b.prime for b in beats}) == 3 and len({b.key for b in beats}) == 3
    assert all(b.prime.bit_length() == 256 and b.sectors == 10 and host_is_prime(b.prime) for b in beats)
    datas = [hashlib.sha256(b"owner %d" % i).digest() * (40 + 13 * i) + b"tail" for i in range(3)]
    enc = PySwizzle.encode_mixed([(b, io.BytesIO(d)) for b, d in zip(beats, datas)])
    chals = [b.gen_challenge(state) for b, (_, state) in zip(beats, enc)]
    proofs = PySwizzle.prove_mixed([(b.get_public(), io.BytesIO(d), c, tag)
                                    for b, d, c, (tag, _) in zip(beats, datas, chals, enc)])
    ok = PySwizzle.verify_mixed([(b, pr, c, state) for b, pr, c, (_, state) in zip(beats, proofs, chals, enc)])
    assert ok == [True, True, True]
    # each owner's own loop agrees, and a foreign proof does not verify
    assert beats[0].verify(proofs[0], chals[0], enc[0][1]) is True
    assert beats[0].verify(proofs[1], chals[0], enc[0][1]) is False


def test_heartbeat_generate_many_end_to_end():
    import heartbeat
    import heartbeat_amd
    assert heartbeat.Heartbeat.generate_many.__func__ is heartbeat_amd.Swizzle.Swizzle.generate_many.__func__
    beats = heartbeat.Heartbeat.generate_many(2)
    assert len(beats) == 2 and beats[0].prime != beats[1].prime and beats[0].k_enc != beats[1].k_enc
    assert all(isinstance(b, heartbeat.Heartbeat) and b.prime.bit_length() == 1024 and host_is_prime(b.prime)
               and b.sectors == 10 and b.check_fraction == 1.0 for b in beats)
    datas = [hashlib.sha256(b"cxx owner %d" % i).digest() * (300 + 77 * i) + b"x" for i in range(2)]
    B = heartbeat.Heartbeat
    enc = B.encode_mixed([(b, io.BytesIO(d)) for b, d in zip(beats, datas)])
    chals = [b.gen_challenge(state) for b, (_, state) in zip(beats, enc)]
    proofs = B.prove_mixed([(b.get_public(), io.BytesIO(d), c, tag)
                            for b, d, c, (tag, _) in zip(beats, datas, chals, enc)])
    ok = B.verify_mixed([(b, pr, c, state) for b, pr, c, (_, state) in zip(beats, proofs, chals, enc)])
    assert ok == [True, True]
    assert heartbeat.Heartbeat.generate_many(0) == []
