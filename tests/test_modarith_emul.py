"""The shared lane arithmetic of every kernel -- hb_mac, hb_redc, hb_to_mont
and hb_reduce_small (heartbeat_amd/csrc/hb_lane.hpp) -- compiled as plain C++
(tests/emul/emul.cpp) against Python int arithmetic, for NL = 2, 8, 16, 32, 64.

The golden encode cases reach these functions with random operands and never
at NL = 2 or 64.  Here the moduli are the edge primes of every width of the
limb class (edge_primes.py) plus three searched primes (top limb 0x80000000,
all-ones middle limbs, seeded random), and the operands sit on the callers'
stated bounds: factors that are not below p (a sector may be one), single bits
and all-ones limbs, and for hb_reduce_small every q p + r around the quotient
estimate's rounding points up to the last value of its domain, 2^32 p - 1.
Everything is bit-exact.
"""
import ctypes
import functools
import importlib
import os
import random
import subprocess

import numpy as np
import pytest

import edge_primes as E

HERE = os.path.dirname(os.path.abspath(__file__))
NLS = (2, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("modarith") / "libhbemul_modarith.so")
    src = os.path.join(HERE, "emul", "emul.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    u32p, c = ctypes.POINTER(ctypes.c_uint32), ctypes
    L.emul_mont_mul.argtypes = [c.c_int, u32p, c.c_uint32, u32p, u32p, u32p]
    L.emul_to_mont.argtypes = [c.c_int, u32p, c.c_uint32, u32p, u32p]
    L.emul_reduce_small.argtypes = [c.c_int, u32p, c.c_uint32, u32p, u32p]
    L.emul_mac_sum.argtypes = [c.c_int, u32p, c.c_uint32, u32p, u32p, u32p, u32p]
    return L


# ------------------------------------------------------------------ limbs
def limbs(vals, nl):
    """ints -> a C-contiguous uint32 array of len(vals) x nl little-endian limbs."""
    raw = b"".join(v.to_bytes(4 * nl, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u4").astype(np.uint32).reshape(len(vals), nl).copy()


def ints(arr):
    nl = arr.shape[1]
    raw = arr.astype("<u4").tobytes()
    return [int.from_bytes(raw[4 * nl * k:4 * nl * (k + 1)], "little") for k in range(arr.shape[0])]


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


# ------------------------------------------------------------------ moduli
@functools.lru_cache(maxsize=None)
def searched_primes(nl):
    """[(label, p)]: three primes of exactly 32 nl bits found by a seeded
    search over odd candidates with the project's Miller-Rabin test."""
    is_prime = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")._is_probable_prime
    rng = random.Random(0xED6E0000 + nl)
    bits = 32 * nl

    def first_prime(n):
        n |= 1
        while not is_prime(n):
            n += 2
        return n

    # top limb 0x80000000, random lower limbs (the step stays in the low limbs)
    top = first_prime((0x80000000 << (bits - 32)) | rng.getrandbits(bits - 32))
    assert top >> (bits - 32) == 0x80000000
    # all-ones middle limbs between a random top and bottom limb (none at nl = 2)
    mid = ((1 << (bits - 64)) - 1) << 32
    ones = first_prime(((rng.getrandbits(32) | 0x80000000) << (bits - 32)) | mid | (rng.getrandbits(32) & 0x7FFFFFFF))
    assert ones & mid == mid
    rnd = first_prime(rng.getrandbits(bits) | (1 << (bits - 1)))
    assert top.bit_length() == ones.bit_length() == rnd.bit_length() == bits
    return [("top80", top), ("ones", ones), ("random", rnd)]


def moduli(nl):
    out = [("%s%d" % (w, b), p) for b in E.NL_BITS[nl] for w, p in E.pair(b)]
    return out + searched_primes(nl)


def special_operands(nl, p):
    """The issue's operand list: 0, 1, 2, p - 1, p, p + 1, 2^(32 nl) - 1, a
    single set bit in each limb, all-ones in one limb."""
    R = 1 << (32 * nl)
    out = [0, 1, 2, p - 1, p, p + 1, R - 1]
    for t in range(nl):
        out.append(1 << (32 * t + (7 * t + 3) % 32))
        out.append(0xFFFFFFFF << (32 * t))
    return [x for x in out if x < R]


# ------------------------------------------------------------------ Montgomery product
@pytest.mark.parametrize("nl", NLS)
def test_montgomery_product(emul, nl):
    """hb_mac + hb_redc + hb_reduce_small == a b R^-1 mod p.

    hb_block_tag's contract is a < p (alpha in Montgomery form) and any b
    below R (a sector, possibly >= p); then T = a b < p R and REDC's
    v < T / R + p < 2 p.  Every such pair is compared.  Pairs with both factors
    >= p are compared as well wherever v stays inside hb_reduce_small's
    documented domain, T / R + p <= 2^32 p; a narrow prime in a wide limb class
    (32 bits at NL = 2, 128 at 8, 384 at 16) has pairs outside it, which no
    kernel forms, and those are counted, not compared."""
    R = 1 << (32 * nl)
    for label, p in moduli(nl):
        rng = random.Random(p & 0xFFFFFFFF)
        sp = special_operands(nl, p)
        rnd = [rng.getrandbits(32 * nl) for _ in range(200)]
        pairs = [(a, b) for a in sp for b in sp]
        pairs += [(rnd[i], rnd[(i + 1) % 200]) for i in range(200)]
        pairs += [(rnd[i] % p, sp[i % len(sp)]) for i in range(200)]
        pairs += [(sp[i % len(sp)], rnd[i]) for i in range(200)]
        dom = [(a, b) for a, b in pairs if (a * b >> (32 * nl)) + p <= (p << 32)]
        domset = set(dom)
        assert all((a, b) in domset for a, b in pairs if a < p)   # the kernels' contract is inside
        assert len(dom) * 2 > len(pairs)
        if R <= ((1 << 32) - 1) * p:
            assert len(dom) == len(pairs)
        a, b = limbs([x for x, _ in dom], nl), limbs([y for _, y in dom], nl)
        out = np.zeros_like(a)
        assert emul.emul_mont_mul(nl, ptr(limbs([p], nl)), len(dom), ptr(a), ptr(b), ptr(out)) == 0
        rinv = pow(R, -1, p)
        got = ints(out)
        for k, (x, y) in enumerate(dom):
            assert got[k] == x * y * rinv % p, (nl, label, hex(x), hex(y))


@pytest.mark.parametrize("nl", NLS)
def test_to_mont(emul, nl):
    """hb_to_mont(x) == x R mod p for every x below R (operands >= p included)."""
    R = 1 << (32 * nl)
    for label, p in moduli(nl):
        rng = random.Random((p >> 7) & 0xFFFFFFFF)
        xs = special_operands(nl, p) + [rng.getrandbits(32 * nl) for _ in range(200)]
        x = limbs(xs, nl)
        out = np.zeros_like(x)
        assert emul.emul_to_mont(nl, ptr(limbs([p], nl)), len(xs), ptr(x), ptr(out)) == 0
        got = ints(out)
        for k, v in enumerate(xs):
            assert got[k] == v * R % p, (nl, label, hex(v))


# ------------------------------------------------------------------ hb_reduce_small
QS = (0, 1, 2, 3, 1 << 16, 1 << 29, 3 * (1 << 29) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1)


def reduce_inputs(p):
    """v = q p + r for r in {0, 1, p - 1}, and q p - 1, at the quotients where
    the double estimate, its floor and the u32 conversion can go wrong; 500
    seeded random v below 2^32 p.  The last value of the documented domain,
    2^32 p - 1 (q = 2^32 - 1, r = p - 1), is among them: there the estimate
    rounds to 2^32."""
    vs = []
    for q in QS:
        vs += [q * p, q * p + 1, q * p + p - 1]
        if q:
            vs.append(q * p - 1)
    rng = random.Random((p >> 3) & 0xFFFFFFFF)
    vs += [rng.randrange(p << 32) for _ in range(500)]
    assert (p << 32) - 1 in vs and all(0 <= v < p << 32 for v in vs)
    return vs


@pytest.mark.parametrize("nl", NLS)
def test_reduce_small_whole_domain(emul, nl):
    """hb_reduce_small(v) == v % p for v < 2^32 p, the stated domain, its last
    value included (every caller's bound -- (S + 2) p, T + F < 2^32 p of the
    split MAC, 2 p of hb_to_mont -- lies inside it)."""
    for label, p in moduli(nl):
        vs = reduce_inputs(p)
        v = limbs(vs, nl + 1)
        out = np.zeros((len(vs), nl), dtype=np.uint32)
        assert emul.emul_reduce_small(nl, ptr(limbs([p], nl)), len(vs), ptr(v), ptr(out)) == 0
        got = ints(out)
        for k, x in enumerate(vs):
            assert got[k] == x % p, (nl, label, "q=%d r=%d" % divmod(x, p))


# ------------------------------------------------------------------ accumulate, reduce once
@pytest.mark.parametrize("nl", NLS)
@pytest.mark.parametrize("S", [1, 2, 16, 2048])
def test_accumulate_then_reduce_once(emul, nl, S):
    """hb_block_tag's shape at its largest operands: S products of
    (p - 1) (2^(32 NL) - 1) on top of F = p - 1 in the 2 NL + 1 limb
    accumulator, one hb_redc and one hb_reduce_small.  hb_block_tag states
    acc < (S + 1) p R and REDC(acc) < (S + 2) p, so the sector count is
    bounded only by (S + 2) p <= 2^32 p; 2048 (HB_MFMA_MAX_S, a 64 KiB block
    of a 256-bit prime) is the largest the kernels are run with, and
    test_reduce_small_whole_domain covers the bound's far end."""
    R = 1 << (32 * nl)
    for label, p in moduli(nl):
        a = limbs([p - 1] * S, nl)
        b = limbs([R - 1] * S, nl)
        F = limbs([p - 1], nl)
        out = np.zeros((1, nl), dtype=np.uint32)
        assert emul.emul_mac_sum(nl, ptr(limbs([p], nl)), S, ptr(a), ptr(b), ptr(F), ptr(out)) == 0
        want = (p - 1 + S * (p - 1) * (R - 1) * pow(R, -1, p)) % p
        assert ints(out)[0] == want, (nl, label, S)


@pytest.mark.parametrize("nl", NLS)
def test_accumulate_mixed_operands(emul, nl):
    """The same shape with distinct operands per product: a_j below p (special
    and random), b_j any sector value, F random below p."""
    R = 1 << (32 * nl)
    for label, p in moduli(nl):
        rng = random.Random((p >> 11) & 0xFFFFFFFF)
        sp = special_operands(nl, p)
        av = [x % p for x in sp] + [rng.randrange(p) for _ in range(16)]
        bv = [sp[(3 * j + 1) % len(sp)] for j in range(len(sp))] + [rng.getrandbits(32 * nl) for _ in range(16)]
        f = rng.randrange(p)
        out = np.zeros((1, nl), dtype=np.uint32)
        assert emul.emul_mac_sum(nl, ptr(limbs([p], nl)), len(av), ptr(limbs(av, nl)), ptr(limbs(bv, nl)),
                                 ptr(limbs([f], nl)), ptr(out)) == 0
        want = (f + sum(x * y for x, y in zip(av, bv)) * pow(R, -1, p)) % p
        assert ints(out)[0] == want, (nl, label)
