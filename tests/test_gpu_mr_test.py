"""hb_mr_test on the GPU against sprp() written with pow()
(tests/prime_vectors.py): the emulation's vector set, one call per width;
mixed bit lengths in one call; rounds 1 and 5; rejected arguments leave the
verdict buffer untouched; and the context still encodes afterwards."""
import ctypes
import io
import random

import pytest

import prime_vectors as pv

pytestmark = pytest.mark.gpu

HB_EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from heartbeat_amd import multi
    return multi.primary_context()


def raw_mr_test(ctx, width, cands, bases, rounds, fill=0xAA):
    """hb_mr_test through ctypes: (rc, verdict bytes, last error); the
    verdict buffer starts as `fill`."""
    from heartbeat_amd import _native
    L = _native.lib()
    cb = b"".join(n.to_bytes(width, "big") for n in cands)
    bb = b"".join(a.to_bytes(width, "big") for a in bases)
    out = ctypes.create_string_buffer(bytes([fill]) * (len(cands) + 1), len(cands) + 1)
    with ctx.lock:
        rc = L.hb_mr_test(ctx.h, cb, width, len(cands), bb, rounds, out)
        err = L.hb_last_error(ctx.h).decode()
    return rc, out.raw[:len(cands)], err


def test_vector_set_one_call_per_width(ctx):
    by_width = {}
    for width, n, bases in pv.vectors():
        by_width.setdefault(width, []).append((n, bases))
    assert {pv.nl_of_width(w) for w in by_width} == {2, 8, 16, 32, 64}
    for width, items in sorted(by_width.items()):
        # a candidate per (n, base), rounds = 1: a verdict per pair
        cands = [n for n, bases in items for _ in bases]
        flat = [a for _, bases in items for a in bases]
        rc, got, err = raw_mr_test(ctx, width, cands, flat, 1)
        assert rc == 0, err
        want = bytes(int(pv.sprp(n, a)) for n, a in zip(cands, flat))
        assert got == want, (width, [(hex(n), hex(a)) for n, a, g, w in zip(cands, flat, got, want) if g != w][:3])
        if pv.nl_of_width(width) == 64:
            continue   # (the 2048-bit class is slow: the grouping is checked on the others)
        # and all four bases of a candidate as one verdict
        rc, got, err = raw_mr_test(ctx, width, [n for n, _ in items], flat, 4)
        assert rc == 0, err
        assert got == bytes(int(all(pv.sprp(n, a) for a in bases)) for n, bases in items)


def test_mixed_bit_lengths_rounds_1_and_5(ctx):
    from heartbeat_amd import primes
    rng = random.Random(11)
    cands = [pv.prime_of(b) for b in (8, 33, 64, 65, 129, 256, 257, 512, 1000, 1024)]
    cands += [rng.getrandbits(b) | (1 << (b - 1)) | 1 for b in (9, 40, 100, 300, 700, 1024)]
    cands += [2047, 3215031751, 561, 5, pv.prime_of(20) ** 2]
    for rounds in (1, 5):
        bases = [[2, 3, 5, 7, n - 2][:rounds] if n > 9 else [2, n - 2, 2, n - 2, 2][:rounds] for n in cands]
        got = primes.mr_test(cands, bases)
        assert got == [all(pv.sprp(n, a) for a in row) for n, row in zip(cands, bases)], rounds
    # the exact function, not "is prime"
    assert primes.mr_test([3215031751], [[2, 3, 5, 7]]) == [True]
    assert primes.mr_test([3215031751], [[2, 3, 5, 7, 11]]) == [False]
    assert primes.mr_test([], []) == []


@pytest.mark.parametrize("cands,bases,rounds,word", [
    ([101, 100, 103], [2, 2, 2], 1, "candidate 1"),          # even candidate
    ([101, 3], [2, 2], 1, "candidate 1"),                     # below 5
    ([1, 101], [2, 2], 1, "candidate 0"),
    ([101, 103], [2, 1], 1, "candidate 1"),                   # base of 1
    ([101, 103], [2, 0], 1, "candidate 1"),
    ([101, 103], [100, 2], 1, "candidate 0"),                 # base of n - 1
    ([101, 103], [99, 2, 2, 103], 2, "candidate 1"),          # base of n
    ([101, 103], [], 0, "rounds"),                            # rounds of 0
])
def test_rejected_arguments_write_nothing(ctx, cands, bases, rounds, word):
    for width in (1, 4, 9, 128):
        rc, got, err = raw_mr_test(ctx, width, cands, bases, rounds)
        assert rc == HB_EINVAL and word in err, (rc, err)
        assert got == b"\xaa" * len(cands)


def test_width_257_unsupported_and_context_still_encodes(ctx, golden_encode):
    from heartbeat_amd import _native
    rc, got, err = raw_mr_test(ctx, 257, [101], [2], 1)
    assert rc == _native.HB_EUNSUPPORTED and got == b"\xaa"
    rc, got, err = raw_mr_test(ctx, 256, [101, 561], [2, 2], 1)
    assert rc == 0 and got == b"\x01\x00", err
    rc, got, err = raw_mr_test(ctx, 8, [], [], 3)
    assert rc == 0
    # the context is still usable: one golden encode
    import importlib
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    c = next(c for c in golden_encode["cases"] if len(c["tags"]) > 3)
    tag, _ = pys.encode_file(int(c["prime"], 16), c["sectors"], bytes.fromhex(c["f_key"]),
                             bytes.fromhex(c["alpha_key"]), io.BytesIO(bytes.fromhex(c["data"])))
    assert tag.sigma == [int(t, 16) for t in c["tags"]], c["name"]
