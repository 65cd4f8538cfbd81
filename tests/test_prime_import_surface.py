"""The prime entries' surface: the ctypes signatures, getPrimes beside getPrime
under the reference's import paths, generate_many on both classes, and --
without a GPU -- HeartbeatError from every call that needs one."""
import ctypes
import importlib
import os

import pytest

from conftest import ROOT


def test_native_binding_lists_the_prime_calls():
    from heartbeat_amd import _native
    sig = {s[0]: s for s in _native.SIGNATURES}
    c = ctypes
    assert sig["hb_mr_test"][1:] == (c.c_int, [c.c_void_p, c.c_char_p, c.c_size_t, c.c_uint64, c.c_char_p,
                                               c.c_uint32, c.c_void_p])
    assert sig["hb_prime_search"][1:] == (c.c_int, [c.c_void_p, c.c_uint32, c.c_char_p, c.c_uint64, c.c_uint32,
                                                    c.c_char_p, c.c_uint32, c.c_void_p, c.c_void_p,
                                                    c.POINTER(c.c_uint64)])
    with open(os.path.join(ROOT, "include", "hbswizzle.h")) as fh:
        header = " ".join(fh.read().split())
    assert ("int hb_mr_test(hb_ctx *ctx, const uint8_t *cands_be, size_t width, uint64_t ncands, "
            "const uint8_t *bases_be, uint32_t rounds, uint8_t *verdicts);") in header
    assert ("int hb_prime_search(hb_ctx *ctx, uint32_t bits, const uint8_t *starts_be, uint64_t nstarts, "
            "uint32_t window, const uint8_t *bases_be, uint32_t rounds, uint8_t *primes_be, uint8_t *found, "
            "uint64_t *tests_out);") in header
    assert "3215031751" in header


def test_getprimes_and_generate_many_reexported():
    amd = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    hb_mod = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    primes = importlib.import_module("heartbeat_amd.primes")
    import heartbeat
    import heartbeat_amd
    assert "getPrimes" in amd.__all__ and "getPrime" in amd.__all__
    assert "getPrimes" in hb_mod.__all__ and hb_mod.getPrimes is amd.getPrimes is primes.getPrimes
    assert set(primes.__all__) == {"mr_test", "prime_search", "getPrimes"}
    assert callable(amd.PySwizzle.generate_many) and callable(heartbeat_amd.Swizzle.Swizzle.generate_many)
    assert heartbeat.PySwizzle.PySwizzle.generate_many is amd.PySwizzle.generate_many
    assert heartbeat.Heartbeat.generate_many.__func__ is heartbeat_amd.Heartbeat.generate_many.__func__
    assert "long gaps" in " ".join(primes.getPrimes.__doc__.split()) and "OpenSSL" in primes.getPrimes.__doc__
    # nothing to draw: no GPU needed
    assert primes.getPrimes(1024, 0) == [] and amd.PySwizzle.generate_many(0) == []
    assert heartbeat.Heartbeat.generate_many(0) == []


def have_gpu():
    from heartbeat_amd import multi
    try:
        return multi.visible_device_count() > 0
    except Exception:
        return False


def test_without_a_gpu_the_calls_raise_heartbeat_error():
    if have_gpu():
        pytest.skip("a GPU is present: tests/test_gpu_getprimes.py runs the calls")
    from heartbeat_amd import HeartbeatError, primes
    amd = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    import heartbeat
    for call in (lambda: primes.mr_test([101], [[2]]),
                 lambda: primes.prime_search(8, [129], [[3]], 5),
                 lambda: primes.getPrimes(64, 1),
                 lambda: amd.PySwizzle.generate_many(1, primebits=64),
                 lambda: heartbeat.Heartbeat.generate_many(1)):
        with pytest.raises(HeartbeatError):
            call()
    # the host path is untouched
    assert amd.getPrime(64).bit_length() == 64
