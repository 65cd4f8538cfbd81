"""CPU tests of the batched cxx encode's Python layer (heartbeat_amd.Swizzle:
encode_files, Swizzle.encode_many = heartbeat.Heartbeat().encode_many) over a
small stand-in for libhbswizzle.so whose hb_cxx_encode_many and hb_encode
delegate to the oracle's cxx restatement -- no GPU.

Reference: a caller's loop over Swizzle.encode (cxx/shacham_waters_private.cxx:
638-702: fresh keys per file, the file read from its position to EOF, the state
encrypted and signed)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S


class CxxLib(object):
    """The entry points Swizzle.encode and encode_files reach: a context,
    hb_cxx_encode_many and hb_encode(HB_PRF_CXX) over the oracle, and a
    reversible stand-in for the State's AES.  `log` records every call that
    would run on the GPU."""

    def __init__(self):
        self.log = []

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

    def hb_aes_cfb128(self, key, klen, iv, data, out, n, encrypt):
        pad = (bytes(key[:klen]) + bytes(iv[:16])) * (n // 16 + 1)
        ctypes.memmove(out, bytes(a ^ b for a, b in zip(bytes(data[:n]), pad)), n)
        return 0

    @staticmethod
    def _tags(p, sectors, fk, ak, data):
        from oracle import oracle as O
        w = (p.bit_length() + 7) // 8
        return b"".join(t.to_bytes(w, "big") for t in O.cxx_encode(p, sectors, fk, ak, data))

    def hb_cxx_encode_many(self, h, pb, plen, sectors, klen, descs, n, flags, tries):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("many", int(n), int(klen), int(flags)))
        for i in range(n):
            # the struct's raw words: f_key, alpha_key, data, len, tags
            words = (ctypes.c_uint64 * 5).from_address(ctypes.addressof(descs[i]))
            fk, ak = ctypes.string_at(words[0], klen), ctypes.string_at(words[1], klen)
            data = ctypes.string_at(words[2], words[3]) if words[3] else b""
            raw = self._tags(p, sectors, fk, ak, data)
            ctypes.memmove(words[4], raw, len(raw))
        tries._obj.value = 0
        return 0

    def hb_encode(self, h, pb, plen, sectors, fk, ak, klen, block_base, data, length, nblocks, tags, flags, tries):
        from heartbeat_amd import _native
        assert flags & _native.HB_PRF_CXX and block_base == 0
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("single", int(length)))
        addr = data if isinstance(data, int) else getattr(data, "value", None)
        blob = ctypes.string_at(addr, int(length)) if length else b""
        raw = self._tags(p, sectors, bytes(fk[:klen]), bytes(ak[:klen]), blob)
        dst = tags if isinstance(tags, int) else tags.value
        ctypes.memmove(dst, raw, len(raw))
        return 0


@pytest.fixture
def swz():
    return importlib.import_module("heartbeat_amd.Swizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = CxxLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


def _keyed(swz, monkeypatch, keys):
    """_random_bytes hands out `keys` for 32-byte draws (f_key, alpha_key per
    file, in file order) and a fixed IV."""
    queue = list(keys)
    monkeypatch.setattr(swz, "_random_bytes", lambda n: queue.pop(0) if n == 32 else b"\x07" * n)
    return queue


class Unreadable(object):
    def read(self, *a):
        raise IOError("no such medium")

    def tell(self):
        return 0


def test_encode_many_equals_the_loop(lib, oracle, swz, monkeypatch, tmp_path):
    blobs = [b"", b"q" * (C - 1), b"r" * C, bytes(range(200)) * 5, b"tail" * 99]
    skips = [0, 0, 3, 0, 5]
    keys = [bytes([i + 1]) * 32 for i in range(2 * len(blobs))]
    beat = swz.Swizzle(sectors=S, prime=P256)
    path = tmp_path / "real.bin"
    path.write_bytes(blobs[4])

    def files():
        fs = [io.BytesIO(b) for b in blobs[:4]] + [open(str(path), "rb")]
        for f, k in zip(fs, skips):
            f.seek(k)
        return fs

    queue = _keyed(swz, monkeypatch, keys)
    fs = files()
    try:
        res = beat.encode_many(fs)
        ends = [f.tell() for f in fs]
    finally:
        fs[4].close()
    assert queue == [] and lib.log == [("many", 5, 32, 0)]
    queue = _keyed(swz, monkeypatch, keys)
    fs = files()
    try:
        loop = [beat.encode(f) for f in fs]
        assert ends == [f.tell() for f in fs] == [len(b) for b in blobs]     # left at EOF, as encode leaves them
    finally:
        fs[4].close()
    assert lib.log[1:] == [("single", len(b) - k) for b, k in zip(blobs, skips)]
    for k, (blob, skip, (tag, state), (tag1, state1)) in enumerate(zip(blobs, skips, res, loop)):
        rest = blob[skip:]
        assert tag.sigma == tag1.sigma == oracle.cxx_encode(P256, S, keys[2 * k], keys[2 * k + 1], rest), k
        assert state.encrypted and state.__getstate__() == state1.__getstate__()   # same keys, same IV
        assert state.n == len(rest) // C + 1 == len(tag)
        s = state._copy()
        assert s._check_sig_and_decrypt(beat.k_enc, beat.k_mac)
        assert (s.f_key, s.alpha_key) == (keys[2 * k], keys[2 * k + 1])           # fresh keys per file, in order


def test_errors_are_raised_before_any_gpu_work(lib, swz):
    f = [io.BytesIO(b"abc"), io.BytesIO(b"def")]
    for beat in (swz.Swizzle(sectors=0, prime=P256), swz.Swizzle(sectors=S, prime=127)):
        with pytest.raises(HeartbeatError):
            beat.encode_many(f)
        with pytest.raises(HeartbeatError):                                      # what the loop raises
            [beat.encode(x) for x in f]
    keys = [(b"a" * 32, b"b" * 32)] * 2
    with pytest.raises(HeartbeatError):
        swz.encode_files(P256, S, keys[:1], f)                                   # key list of the wrong length
    with pytest.raises(HeartbeatError):
        swz.encode_files(P256, S, [keys[0], (b"a" * 16, b"b" * 16)], f)          # unequal key lengths
    with pytest.raises(HeartbeatError):
        swz.encode_files(P256, 0, keys, f)
    with pytest.raises(HeartbeatError):
        swz.encode_files(127, S, keys, f)
    assert lib.log == []
    assert [x.tell() for x in f] == [0, 0]


def test_unreadable_file_raises_at_its_item(lib, swz):
    beat = swz.Swizzle(sectors=S, prime=P256)
    fs = [io.BytesIO(b"x" * 300), io.BytesIO(b"y" * 10), Unreadable(), io.BytesIO(b"z" * 50)]
    with pytest.raises(IOError):
        beat.encode_many(fs)
    assert lib.log == []                                                         # no GPU call at all
    after_many = [f.tell() for f in fs]
    fs2 = [io.BytesIO(b"x" * 300), io.BytesIO(b"y" * 10), Unreadable(), io.BytesIO(b"z" * 50)]
    with pytest.raises(IOError):
        [beat.encode(f) for f in fs2]
    # the loop has encoded the files before the bad one and not touched the one after
    assert [f.tell() for f in fs2] == after_many == [300, 10, 0, 0]
    assert lib.log == [("single", 300), ("single", 10)]


def test_below_the_minimum_the_single_method_runs(lib, oracle, swz, monkeypatch):
    beat = swz.Swizzle(sectors=S, prime=P256)
    assert swz.CXX_ENCODE_MANY_MIN >= 1
    assert beat.encode_many([]) == [] and swz.encode_files(P256, S, [], []) == []
    assert lib.log == []
    n = swz.CXX_ENCODE_MANY_MIN
    blobs = [bytes([65 + i]) * (100 + i) for i in range(n)]
    keys = [bytes([i + 1]) * 32 for i in range(2 * n)]
    queue = _keyed(swz, monkeypatch, keys)
    res = beat.encode_many([io.BytesIO(b) for b in blobs[:n - 1]])
    assert lib.log == [("single", len(b)) for b in blobs[:n - 1]]
    assert [t.sigma for t, _ in res] == [oracle.cxx_encode(P256, S, keys[2 * k], keys[2 * k + 1], blobs[k])
                                         for k in range(n - 1)]
    del lib.log[:]
    queue[:] = keys
    res = beat.encode_many([io.BytesIO(b) for b in blobs])
    assert lib.log == [("many", n, 32, 0)]
    assert [t.sigma for t, _ in res] == [oracle.cxx_encode(P256, S, keys[2 * k], keys[2 * k + 1], blobs[k])
                                         for k in range(n)]


def test_reexported_through_heartbeat(swz):
    import heartbeat
    hb = importlib.import_module("heartbeat.Swizzle")
    assert heartbeat.Heartbeat is hb.Swizzle is swz.Swizzle
    assert hasattr(heartbeat.Heartbeat, "encode_many")
