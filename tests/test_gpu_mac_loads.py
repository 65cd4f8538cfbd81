"""GPU parity of the matrix-core MACs' file loads (hb_mac_src.hpp: every piece
is loaded unconditionally, a lane without a block from the A-fragment buffer).
Tags byte-equal to the CPU oracle (reference: PySwizzle.py:279-314,
util.py:83-96) for the shapes at which a wave has lanes without a block:

* 256-bit prime: the 16x16x64 path at S = 2 (one K slice), 6 (a pair plus an
  odd slice) and 16 (the bench shape); the sector-load path at S = 3 and 5; the
  32x32x32 whole-line path at S = 4 ($HB_MFMA_LINE32);
* 1, 63, 65 and 257 whole blocks plus a last block of 1 and of C - 1 bytes, a
  file shorter than a block, an empty file, and a block_base != 0;
* every file encoded twice on one context with the digest table on (the
  storing, then the loading first-pass kernel) and once with it off;
* a seeded 1024-bit prime at S = 10 over the same block counts (the split
  wide-prime MAC, hb_wide.hpp, whose loads keep their conditional form).

$HB_NO_SMALL_ENCODE puts these small files on the two-pass kernels."""
import hashlib

import numpy as np
import pytest

from test_gpu_digest_cache import dev_encode
from test_gpu_parity import P256
from test_gpu_wide import _prime

pytestmark = pytest.mark.gpu

GIB = 1 << 30
NFULL = (1, 63, 65, 257)


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture()
def ctx(nat, monkeypatch):
    monkeypatch.setenv("HB_NO_SMALL_ENCODE", "1")
    return nat.context(0, instance=8)


def files(C):
    """(label, length, block_base) of the files of one shape."""
    out = [("n%d+%d" % (n, t), n * C + t, 0) for n in NFULL for t in (1, C - 1)]
    out += [("short", 37, 0), ("empty", 0, 0), ("based", 65 * C + 1, 2 ** 32 - 30)]   # (C >= 64)
    return out


def check_shape(nat, ctx, oracle, p, S, tag):
    C = (p.bit_length() // 8) * S
    rng = np.random.default_rng(1000 * S + p.bit_length())
    for label, n, base in files(C):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        fk = hashlib.sha256(b"ml-f-%s-%s" % (tag, label.encode())).digest()
        ak = hashlib.sha256(b"ml-a-%s-%s" % (tag, label.encode())).digest()
        want = oracle.encode(p, S, fk, ak, data, block_base=base)
        ctx.set_digest_cache(0)
        ctx.set_digest_cache(8 * GIB)
        try:
            for mode in ("store", "load", "none"):
                if mode == "none":
                    ctx.set_digest_cache(0)
                got, _ = dev_encode(nat, ctx, p, S, fk, ak, data, base)
                assert ctx.digest_cache_info()["last_mode"] == mode, (tag, label, mode)
                assert got == want, (tag, label, mode)
        finally:
            ctx.set_digest_cache(8 * GIB)


@pytest.mark.parametrize("S,switch", [(2, None), (6, None), (16, None),        # 16x16x64
                                      (3, None), (5, None),                    # sector loads (S odd)
                                      (4, "HB_MFMA_LINE32")])                  # 32x32x32 whole lines
def test_mfma_mac_lanes_without_a_block(nat, ctx, oracle, monkeypatch, S, switch):
    monkeypatch.setenv("HB_MFMA_MIN_S", "2")   # the MFMA MAC below 4 sectors too
    if switch:
        monkeypatch.setenv(switch, "1")
    check_shape(nat, ctx, oracle, P256, S, b"256-%d" % S)


def test_wide_mac_blocks_without_data(nat, ctx, oracle):
    check_shape(nat, ctx, oracle, _prime(1024, 20261), 10, b"1024-10")
