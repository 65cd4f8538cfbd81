"""GPU tests of the context's digest table (hb_digest_cache.hpp, hb_runtime.cpp):
the two-pass encode stores SHA256(str(block index)) of the range it encodes
and later encodes inside that range load the digests instead of hashing.
Every tag is compared with the CPU oracle (reference: PySwizzle.py:279-314,
util.py:83-96), the table's mode and range with hb_ctx_digest_cache_info.
The tests run on a context of their own, with $HB_NO_SMALL_ENCODE so that the
two-pass kernels run at these small sizes."""
import ctypes
import hashlib
import importlib

import numpy as np
import pytest

from test_gpu_parity import P256

pytestmark = pytest.mark.gpu

GIB = 1 << 30


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture()
def ctx(nat, monkeypatch):
    """The tests' own context, its table empty and its cap the default."""
    monkeypatch.setenv("HB_NO_SMALL_ENCODE", "1")
    c = nat.context(0, instance=7)
    c.set_digest_cache(0)
    c.set_digest_cache(8 * GIB)
    info = c.digest_cache_info()
    assert (info["lo"], info["hi"], info["bytes"]) == (0, 0, 0), info
    return c


def keys(label, k):
    return (hashlib.sha256(b"dc-f-%s-%d" % (label, k)).digest(), hashlib.sha256(b"dc-a-%s-%d" % (label, k)).digest())


def file_bytes(seed, p, S, nfull, tail=5):
    C = (p.bit_length() // 8) * S
    return np.random.default_rng(seed).integers(0, 256, nfull * C + tail, dtype=np.uint8).tobytes()


def next_prime(n):
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    n |= 1
    while not pys._is_probable_prime(n):
        n += 2
    return n


class Dev(object):
    def __init__(self, nat, ctx, n):
        self.nat, self.ctx, self.n = nat, ctx, n
        p = ctypes.c_void_p()
        ctx.check(nat.lib().hb_device_malloc(ctx.h, max(n, 1), ctypes.byref(p)))
        self.p = p.value

    def upload(self, data):
        a = np.frombuffer(data, dtype=np.uint8)
        if len(a):
            self.ctx.check(self.nat.lib().hb_memcpy(self.ctx.h, self.p, a.ctypes.data, len(a), 1))

    def download(self):
        out = np.empty(self.n, dtype=np.uint8)
        self.ctx.check(self.nat.lib().hb_memcpy(self.ctx.h, out.ctypes.data, self.p, self.n, 2))
        return out.tobytes()

    def free(self):
        self.ctx.check(self.nat.lib().hb_device_free(self.ctx.h, self.p))


def dev_encode(nat, ctx, p, S, fk, ak, data, base=0):
    """(tags as ints, tries) of a device-resident encode of `data` as blocks base ..."""
    w = nat.width_of(p)
    nb = len(data) // ((p.bit_length() // 8) * S) + 1
    pb = nat.be(p)
    d, t = Dev(nat, ctx, len(data)), Dev(nat, ctx, nb * w)
    try:
        d.upload(data)
        tries = ctypes.c_uint64()
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), base, d.p, len(data), nb, t.p, 3,
                                      ctypes.byref(tries)))
        raw = t.download()
    finally:
        d.free()
        t.free()
    return [int.from_bytes(raw[i:i + w], "big") for i in range(0, len(raw), w)], tries.value


def check_call(nat, ctx, oracle, p, S, label, k, seed, nfull, base, mode, rng=None):
    """One encode with its own keys and file bytes: tags == oracle, the
    table's mode as expected and its valid range `rng` (default: the call's)."""
    fk, ak = keys(label, k)
    data = file_bytes(seed, p, S, nfull)
    got, tries = dev_encode(nat, ctx, p, S, fk, ak, data, base)
    assert got == oracle.encode(p, S, fk, ak, data, block_base=base), (label, k, mode)
    info = ctx.digest_cache_info()
    assert info["last_mode"] == mode, (label, k, info)
    if mode != "none":
        lo, hi = rng if rng else (base, base + nfull + 1)
        assert (info["lo"], info["hi"]) == (lo, hi), (label, k, info)
        assert info["bytes"] >= 32 * (hi - lo)
    return tries


def test_same_range_three_key_pairs(nat, ctx, oracle):
    """Store, load, load over one range with three key pairs and three files:
    the digests are the index's alone."""
    for k, mode in enumerate(("store", "load", "load")):
        check_call(nat, ctx, oracle, P256, 16, b"same", k, 100 + k, 700, 0, mode)


def test_subrange_and_growth(nat, ctx, oracle):
    check_call(nat, ctx, oracle, P256, 16, b"grow", 0, 1, 299, 0, "store")
    # [0, 5000) overlaps [0, 300): a store that extends the range, old entries kept
    check_call(nat, ctx, oracle, P256, 16, b"grow", 1, 2, 4999, 0, "store")
    check_call(nat, ctx, oracle, P256, 16, b"grow", 2, 3, 299, 0, "load", rng=(0, 5000))
    # a range that starts where the table ends extends it upwards, and a
    # request inside the older part then still loads what the first calls stored
    check_call(nat, ctx, oracle, P256, 16, b"grow", 3, 4, 249, 5000, "store", rng=(0, 5250))
    check_call(nat, ctx, oracle, P256, 16, b"grow", 4, 5, 349, 100, "load", rng=(0, 5250))
    check_call(nat, ctx, oracle, P256, 16, b"grow", 5, 6, 299, 4900, "load", rng=(0, 5250))


def test_block_bases_across_decimal_lengths(nat, ctx, oracle):
    """Index ranges whose decimal strings change length and division path
    (lengths 1-3, 5-6, 9-10, across 2^32, 10-11 above 2^32); each is disjoint
    from the one before, so the table is replaced every time."""
    for base in (0, 99990, 999999990, 2 ** 32 - 50, 10 ** 10 - 20):
        check_call(nat, ctx, oracle, P256, 16, b"base", 0, base % 1000, 200, base, "store")
        check_call(nat, ctx, oracle, P256, 16, b"base", 1, base % 1000 + 1, 200, base, "load")


def test_cap_below_the_need_and_cap_zero(nat, ctx, oracle):
    ctx.set_digest_cache(32 * 400)            # 401 blocks need 32 x 401 bytes
    check_call(nat, ctx, oracle, P256, 16, b"cap", 0, 1, 400, 0, "none")
    assert ctx.digest_cache_info()["bytes"] == 0
    ctx.set_digest_cache(32 * 401)
    check_call(nat, ctx, oracle, P256, 16, b"cap", 1, 2, 400, 0, "store")
    # growth past the cap: the union does not fit, the request alone does not either
    check_call(nat, ctx, oracle, P256, 16, b"cap", 2, 3, 500, 0, "none")
    assert (ctx.digest_cache_info()["lo"], ctx.digest_cache_info()["hi"]) == (0, 401)
    check_call(nat, ctx, oracle, P256, 16, b"cap", 3, 4, 400, 0, "load")
    ctx.set_digest_cache(0)
    assert ctx.digest_cache_info() == {"lo": 0, "hi": 0, "bytes": 0, "last_mode": "load"}
    check_call(nat, ctx, oracle, P256, 16, b"cap", 4, 5, 400, 0, "none")
    assert ctx.digest_cache_info()["bytes"] == 0


@pytest.mark.parametrize("early", [True, False])
def test_high_rejection_prime_every_mode(nat, ctx, oracle, monkeypatch, early):
    """The first prime above 2^255 rejects almost half of all tries, so about
    half the blocks go through the retry pass, which reads the table in store
    and load modes; with and without the early retry listing."""
    p = next_prime(1 << 255)
    if not early:
        monkeypatch.setenv("HB_TEST_NO_EARLY_LIST", "1")
    nfull = 600
    ctx.set_digest_cache(0)
    t0 = check_call(nat, ctx, oracle, p, 16, b"rej", 0, 1, nfull, 0, "none")
    ctx.set_digest_cache(8 * GIB)
    t1 = check_call(nat, ctx, oracle, p, 16, b"rej", 0, 1, nfull, 0, "store")
    t2 = check_call(nat, ctx, oracle, p, 16, b"rej", 0, 1, nfull, 0, "load")
    assert t0 == t1 == t2 and t0 > 1.7 * (nfull + 1), (t0, t1, t2)


@pytest.mark.parametrize("bits,S", [(256, 3), (256, 1), (128, 16), (512, 16)])
def test_other_shapes(nat, ctx, oracle, bits, S):
    """The other first-pass instantiations the table is wired into: the VALU
    MAC (S = 3, S = 1), a 128-bit prime, and a 512-bit prime (the split
    wide-prime encode's F-only passes)."""
    p = P256 if bits == 256 else next_prime((1 << (bits - 1)) + (1 << (bits - 3)) + 12345)
    assert p.bit_length() == bits
    label = b"shape%d-%d" % (bits, S)
    for k, mode in enumerate(("store", "load")):
        check_call(nat, ctx, oracle, p, S, label, k, 10 * bits + S + k, 450, 0, mode)


def test_host_input_two_windows(nat, ctx, oracle):
    """300 MiB of host memory at S = 16: two 256 MiB windows, the second
    starting at block 524,288, one table decision for the whole call."""
    p, S, C, w = P256, 16, 512, 32
    n = 300 << 20
    nfull = n // C
    nb = nfull + 1
    data = np.random.default_rng(77).integers(0, 256, n + 9, dtype=np.uint8)
    tags = np.empty(nb * w, dtype=np.uint8)
    pb = nat.be(p)
    spans = [(0, 200), (524288 - 200, 400), (nb - 200, 200)]
    for k, mode in enumerate(("store", "load")):
        fk, ak = keys(b"host", k)
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, 32, 0, data.ctypes.data, len(data), nb,
                                      tags.ctypes.data, 0, None))
        info = ctx.digest_cache_info()
        assert (info["last_mode"], info["lo"], info["hi"]) == (mode, 0, nb), info
        raw = tags.tobytes()
        for b0, cnt in spans:
            want = oracle.encode(p, S, fk, ak, data[b0 * C:(b0 + cnt) * C].tobytes(), block_base=b0, nblocks=cnt)
            got = [int.from_bytes(raw[i * w:(i + 1) * w], "big") for i in range(b0, b0 + cnt)]
            assert got == want, (mode, b0)


def test_async_store_then_encode_of_the_same_range(nat, ctx, oracle):
    """An HB_ASYNC store-mode encode followed at once by a second encode of
    the same range: the second settles the first, whose range is then valid."""
    p, S, w = P256, 16, 32
    nfull = 900
    pb = nat.be(p)
    datas = [file_bytes(40 + k, p, S, nfull) for k in range(2)]
    ks = [keys(b"async", k) for k in range(2)]
    d = [Dev(nat, ctx, len(x)) for x in datas]
    t = [Dev(nat, ctx, (nfull + 1) * w) for _ in range(2)]
    try:
        for k in range(2):
            d[k].upload(datas[k])
        L = nat.lib()
        ctx.check(L.hb_encode(ctx.h, pb, 32, S, ks[0][0], ks[0][1], 32, 0, d[0].p, len(datas[0]), nfull + 1, t[0].p,
                              3 | nat.HB_ASYNC, None))
        ctx.check(L.hb_encode(ctx.h, pb, 32, S, ks[1][0], ks[1][1], 32, 0, d[1].p, len(datas[1]), nfull + 1, t[1].p,
                              3 | nat.HB_ASYNC, None))
        ctx.check(L.hb_ctx_wait(ctx.h, None))
        info = ctx.digest_cache_info()
        assert (info["last_mode"], info["lo"], info["hi"]) == ("load", 0, nfull + 1), info
        for k in range(2):
            raw = t[k].download()
            got = [int.from_bytes(raw[i:i + w], "big") for i in range(0, len(raw), w)]
            assert got == oracle.encode(p, S, ks[k][0], ks[k][1], datas[k]), k
    finally:
        for b in d + t:
            b.free()
