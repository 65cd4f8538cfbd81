"""CPU tests of the batched prove's Python layer (heartbeat_amd.PySwizzle:
prove_files, PySwizzle.prove_many) over a small stand-in for libhbswizzle.so
whose hb_prove_range / hb_prove_many compute mu and sigma with the CPU
oracle's prove -- no GPU.

Reference: a caller's loop over PySwizzle.py:333-370."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S
W = 32


def _prove(p, sectors, ck, chunks, vmax, tags_addr, ntags, data_addr, length):
    """PySwizzle.py:333-370 with the oracle, over raw addresses: bytes of mu | sigma."""
    from oracle import oracle as O
    w = (p.bit_length() + 7) // 8
    tb = ctypes.string_at(tags_addr, ntags * w)
    tags = [int.from_bytes(tb[i * w:(i + 1) * w], "big") for i in range(ntags)]
    data = ctypes.string_at(data_addr, length) if length else b""
    mu, sigma = O.prove(p, sectors, ck, chunks, vmax, tags, data)
    return b"".join(m.to_bytes(w, "big") for m in mu) + sigma.to_bytes(w, "big")


class ProveLib(object):
    """The entry points prove and prove_files reach: a context, the single
    prove (hb_prove_range, whole range) and hb_prove_many reading each
    descriptor's ten raw words."""

    def __init__(self):
        self.calls = []
        self.single = 0

    def hb_ctx_create(self, device, ref):
        ref._obj.value = 1 + device
        return 0

    def hb_ctx_destroy(self, h):
        pass

    def hb_last_error(self, h):
        return b"stand-in"

    def hb_device_count(self, ref):
        ref._obj.value = 1
        return 0

    def hb_prove_range(self, h, pb, plen, sectors, ck, klen, chunks, i0, i1, vmax, vlen, tags, ntags, data, length,
                       flags, mu, sg):
        assert (i0, i1) == (0, chunks) and flags == 0
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.single += 1
        r = _prove(p, sectors, ck[:klen], chunks, int.from_bytes(vmax[:vlen], "big"), tags, ntags, data, length)
        ctypes.memmove(mu, r[:sectors * w], sectors * w)
        ctypes.memmove(sg, r[sectors * w:], w)
        return 0

    def hb_prove_many(self, h, pb, plen, sectors, klen, descs, n, flags):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.calls.append((int(n), int(klen), int(flags)))
        for i in range(n):
            # the struct's raw words: chal_key, chunks, vmax_be, vmax_len, tags,
            # ntags, data, len, mu_out, sigma_out
            x = (ctypes.c_uint64 * 10).from_address(ctypes.addressof(descs[i]))
            r = _prove(p, sectors, ctypes.string_at(x[0], klen), x[1], int.from_bytes(ctypes.string_at(x[2], x[3]), "big"),
                       x[4], x[5], x[6], x[7])
            ctypes.memmove(x[8], r[:sectors * w], sectors * w)
            ctypes.memmove(x[9], r[sectors * w:], w)
        return 0


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def many(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = ProveLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


def _items(pys, oracle, n, cklen=32, first=0):
    """n (file, chal, tag) over files of a few hundred bytes, and their bytes."""
    out = []
    for k in range(first, first + n):
        data = bytes((7 * k + i) & 0xff for i in range(300 + 97 * (k % 5)))
        tags = oracle.encode(P256, S, bytes([k + 1]) * 32, bytes([0x80 + k]) * 32, data)
        tag = pys.Tag()
        tag.sigma = list(tags)
        out.append((io.BytesIO(data), pys.Challenge(len(tags) + k, P256, bytes([0x40 + k]) * cklen), tag))
    return out


def _pairs(proofs):
    return [(x.mu, x.sigma) for x in proofs]


def test_prove_many_equals_loop_of_prove(many, oracle, pys):
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, 5)
    want = [beat.prove(*it) for it in items]
    assert many.single == 5 and many.calls == []
    for (f, chal, tag), x in zip(items, want):                  # the stand-in is the oracle's prove
        assert (x.mu, x.sigma) == tuple(oracle.prove(P256, S, chal.key, chal.chunks, P256, tag.sigma, f.getvalue()))
    got = beat.prove_many(items)
    assert _pairs(got) == _pairs(want)
    assert all(isinstance(g, pys.Proof) for g in got)
    assert many.calls == [(5, 32, 0)]                           # one call, the right count and key length
    assert many.single == 5                                     # and no single call beside it
    assert _pairs(beat.prove_many(iter(items))) == _pairs(want)   # any iterable


def test_prove_files_values(many, oracle, pys):
    (f0, c0, t0), (f1, c1, t1) = _items(pys, oracle, 2, cklen=24)
    got = pys.prove_files(P256, S, [(c0.key, 3, 1000, t0, f0), (c1.key, -2, 77, t1, f1)])
    assert many.calls == [(2, 24, 0)]
    assert got[0] == tuple(oracle.prove(P256, S, c0.key, 3, 1000, t0.sigma, f0.getvalue()))
    assert got[1] == ([0] * S, 0)                               # chunks <= 0: zero sums
    with pytest.raises(HeartbeatError):
        pys.prove_files(P256, S, [(c0.key, 3, 1000, t0, f0), (b"k" * 32, 3, 1000, t1, f1)])   # two key lengths
    with pytest.raises(HeartbeatError) as e:
        pys.prove_files(P256, S, [(c0.key, 3, 1000, pys.Tag(), f0)])
    assert "tag is empty" in str(e.value)
    with pytest.raises(HeartbeatError):
        pys.prove_files(P256, 0, [(c0.key, 3, 1000, t0, f0)])
    assert pys.prove_files(P256, S, []) == []
    assert len(many.calls) == 1


def test_error_order_and_zero_chunks(many, oracle, pys):
    """HeartbeatError("tag is empty") at the first item a loop would raise it
    for, before any library call; chunks <= 0 returns a zero proof first, also
    with an empty tag (PySwizzle.prove's order)."""
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, 4)
    items[1][1].chunks = 0
    items[1] = (items[1][0], items[1][1], pys.Tag())            # zero chunks and an empty tag: a zero proof
    items[3][1].chunks = -1
    want = [beat.prove(*it) for it in items]
    assert _pairs(want)[1] == ([0] * S, 0) and _pairs(want)[3] == ([0] * S, 0)
    singles = many.single
    got = beat.prove_many(items)
    assert _pairs(got) == _pairs(want)
    assert many.calls == [(2, 32, 0)] and many.single == singles   # the zero proofs never reach the library
    items[2] = (items[2][0], items[2][1], pys.Tag())            # an empty tag with chunks > 0
    with pytest.raises(HeartbeatError) as e:
        beat.prove_many(items)
    with pytest.raises(HeartbeatError) as e1:
        [beat.prove(*it) for it in items]
    assert str(e.value) == str(e1.value) == "tag is empty"
    assert len(many.calls) == 1                                 # nothing was sent for the failing batch
    bad = pys.PySwizzle(0, b"K" * 32, P256)
    with pytest.raises(HeartbeatError) as e:
        bad.prove_many(items[:1])
    assert "sectors must be positive" in str(e.value)


def test_minority_key_lengths_go_through_prove(many, oracle, pys):
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, 3) + _items(pys, oracle, 1, cklen=16, first=3) + _items(pys, oracle, 1, first=4) + \
        _items(pys, oracle, 1, cklen=24, first=5)
    got = beat.prove_many(items)
    assert many.calls == [(4, 32, 0)]                           # the majority in one call
    assert many.single == 2                                     # the others through prove()
    assert _pairs(got) == _pairs([beat.prove(*it) for it in items])


def test_sharded_challenges_go_through_prove(many, oracle, pys, monkeypatch):
    """A challenge prove() would shard over several GPUs is not batched."""
    from heartbeat_amd import multi
    monkeypatch.setattr(multi, "_devices", [0, 0])
    monkeypatch.setattr(multi, "MIN_SHARD_CHUNKS", 6)
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, 4)
    for (f, chal, tag), n in zip(items, (3, 5, 12, 4)):
        chal.chunks = n
    got = beat.prove_many(items)
    assert many.calls == [(3, 32, 0)] and many.single == 1      # 12 chunks: through prove()
    for (f, chal, tag), g in zip(items, got):
        assert (g.mu, g.sigma) == tuple(oracle.prove(P256, S, chal.key, chal.chunks, P256, tag.sigma, f.getvalue()))


def test_file_positions_restored(many, oracle, pys, tmp_path):
    """Every file is read whole from its start (absolute offsets,
    PySwizzle.py:353-355) and left where it was."""
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, 3)
    path = tmp_path / "f.bin"
    path.write_bytes(items[2][0].getvalue())
    with open(str(path), "rb") as fh:
        items[2] = (fh, items[2][1], items[2][2])
        items[0][0].seek(11)
        items[1][0].seek(0, io.SEEK_END)
        fh.seek(5)
        got = beat.prove_many(items)
        assert [items[0][0].tell(), fh.tell()] == [11, 5]
        assert items[1][0].tell() == len(items[1][0].getvalue())
        assert many.calls == [(3, 32, 0)]
        assert _pairs(got) == _pairs([beat.prove(*it) for it in items])


def test_descriptor_layout():
    """hb_prove_desc (hbswizzle.h): ten 8-byte words in the header's order."""
    from heartbeat_amd import _native
    D = _native.ProveDesc
    assert ctypes.sizeof(D) == 80
    names = ["chal_key", "chunks", "vmax_be", "vmax_len", "tags", "ntags", "data", "len", "mu_out", "sigma_out"]
    assert [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == list(range(0, 80, 8))
    assert all(getattr(D, n).size == 8 for n in names)
    sig = {name: args for name, _, args in _native.SIGNATURES}["hb_prove_many"]
    assert len(sig) == 8 and sig[5] == ctypes.POINTER(D)


def test_small_batches_go_through_prove(many, oracle, pys):
    """Below PROVE_MANY_MIN items prove() is used."""
    assert pys.PROVE_MANY_MIN == 2
    beat = pys.PySwizzle(S, b"K" * 32, P256)
    items = _items(pys, oracle, pys.PROVE_MANY_MIN)
    few = items[:pys.PROVE_MANY_MIN - 1]
    want = [beat.prove(*it) for it in items]
    singles = many.single
    assert _pairs(beat.prove_many(few)) == _pairs(want[:len(few)])
    assert many.calls == [] and many.single == singles + len(few)
    assert _pairs(beat.prove_many(items)) == _pairs(want)
    assert many.calls == [(len(items), 32, 0)]
    assert beat.prove_many([]) == []


def test_reexported_through_heartbeat(pys):
    hb = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    assert hb.prove_files is pys.prove_files
    assert hasattr(hb.PySwizzle, "prove_many")
