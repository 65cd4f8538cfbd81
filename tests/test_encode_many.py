"""CPU tests of the batched encode's Python layer (heartbeat_amd.PySwizzle:
encode_files, PySwizzle.encode_many) over a small stand-in for libhbswizzle.so
whose hb_encode_many delegates to the CPU oracle -- no GPU.

Reference: a caller's loop over PySwizzle.py:279-311 (encode reads the file
from its current position to EOF, :299, with fresh keys per file, :281)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S


class ManyLib(object):
    """The entry points encode_files reaches: a context, and hb_encode_many
    over the oracle (the State's AES is replaced where a test needs it)."""

    def __init__(self):
        self.calls = []

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

    def hb_encode_many(self, h, pb, plen, sectors, klen, descs, n, flags, tries):
        from oracle import oracle as O
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.calls.append((int(n), int(klen), int(flags)))
        total = 0
        for i in range(n):
            # the struct's raw words: f_key, alpha_key, data, len, tags
            words = (ctypes.c_uint64 * 5).from_address(ctypes.addressof(descs[i]))
            fk, ak = ctypes.string_at(words[0], klen), ctypes.string_at(words[1], klen)
            data = ctypes.string_at(words[2], words[3]) if words[3] else b""
            tags = O.encode(p, sectors, fk, ak, data)
            ctypes.memmove(words[4], b"".join(t.to_bytes(w, "big") for t in tags), len(tags) * w)
            total += len(tags)
        tries._obj.value = total
        return 0


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def many(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = ManyLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


def _keys(n, klen=32):
    return [(bytes([i + 1]) * klen, bytes([0x80 + i]) * klen) for i in range(n)]


def test_encode_files_reads_from_position_to_eof(many, oracle, pys, tmp_path):
    blobs = [bytes(range(256)) * 3 + b"x" * k for k in (0, 1, 77)]
    skips = [0, 5, 300]
    path = tmp_path / "real.bin"
    path.write_bytes(blobs[2])
    files = [io.BytesIO(blobs[0]), io.BytesIO(blobs[1]), open(str(path), "rb")]
    try:
        for f, k in zip(files, skips):
            f.seek(k)
        keys = _keys(3)
        res = pys.encode_files(P256, S, keys, files)
        assert many.calls == [(3, 32, 0)]
        for f, blob, k, (fk, ak), (tag, nblocks) in zip(files, blobs, skips, keys, res):
            rest = blob[k:]
            assert f.tell() == len(blob)                       # left at EOF
            assert nblocks == len(rest) // C + 1 == len(tag)
            assert tag.sigma == oracle.encode(P256, S, fk, ak, rest)
            assert tag._width == 32 and len(bytes(tag.raw(P256))) == nblocks * 32
    finally:
        files[2].close()


def test_encode_files_errors(many, pys):
    f = [io.BytesIO(b"abc"), io.BytesIO(b"def")]
    with pytest.raises(HeartbeatError):
        pys.encode_files(P256, S, _keys(1), f)                 # key list of the wrong length
    with pytest.raises(HeartbeatError):
        pys.encode_files(P256, S, [_keys(1)[0], _keys(1, 16)[0]], f)   # unequal key lengths
    with pytest.raises(HeartbeatError):
        pys.encode_files(P256, S, [(b"a" * 32, b"b" * 16), (b"a" * 32, b"b" * 32)], f)
    with pytest.raises(HeartbeatError):
        pys.encode_files(P256, 0, _keys(2), f)                 # sectors < 1
    with pytest.raises(HeartbeatError):
        pys.encode_files(127, S, _keys(2), f)                  # no whole sector byte (_check)
    beat = pys.PySwizzle(0, b"k" * 32, P256)
    with pytest.raises(HeartbeatError):
        beat.encode_many(f)
    beat = pys.PySwizzle(S, b"k" * 32, 127)
    with pytest.raises(HeartbeatError):
        beat.encode_many(f)
    assert many.calls == []
    assert [x.tell() for x in f] == [0, 0]


def test_empty_list_makes_no_library_call(many, pys):
    assert pys.encode_files(P256, S, [], []) == []
    assert pys.PySwizzle(S, b"k" * 32, P256).encode_many([]) == []
    assert many.calls == []


def test_encode_many_states(many, oracle, pys, monkeypatch):
    from heartbeat_amd import _native

    def xor_cfb8(key, iv, data, encrypt):                      # a reversible stand-in for hb_aes_cfb8
        pad = (bytes(key) + bytes(iv)) * (len(data) // 16 + 1)
        return bytes(a ^ b for a, b in zip(bytes(data), pad))

    monkeypatch.setattr(_native, "aes_cfb8", xor_cfb8)
    blobs = [b"", b"q" * (C - 1), b"r" * C, bytes(range(200)) * 5]
    key = b"K" * 32
    beat = pys.PySwizzle(S, key, P256)
    res = beat.encode_many([io.BytesIO(b) for b in blobs])
    assert many.calls == [(4, 32, 0)]
    seen = set()
    for blob, (tag, state) in zip(blobs, res):
        assert state.encrypted
        state.decrypt(key)
        assert state.chunks == len(blob) // C + 1 == len(tag)
        assert tag.sigma == oracle.encode(P256, S, state.f_key, state.alpha_key, blob)
        seen.add(state.f_key)
        seen.add(state.alpha_key)
    assert len(seen) == 8                                      # fresh keys per file


def test_reexported_through_heartbeat(pys):
    hb = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    assert hb.encode_files is pys.encode_files
    assert hasattr(hb.PySwizzle, "encode_many")
