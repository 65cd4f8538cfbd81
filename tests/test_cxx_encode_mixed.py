"""CPU tests of the cxx mixed-owner encode's Python layer (heartbeat_amd.Swizzle:
encode_files_mixed, Swizzle.encode_mixed = heartbeat.Heartbeat.encode_mixed;
heartbeat_amd._many with the native name and the open_first policy) over a small
stand-in for libhbswizzle.so whose hb_cxx_encode_mixed reads each descriptor's
nine raw words and answers with the oracle's cxx restatement -- no GPU.

Three beats -- a 256-bit prime with S = 16, a 1024-bit one with S = 10, a
61-bit one with S = 3 -- interleaved in one call.

Reference: a loop of b.encode(file) over the beats of many owners
(cxx/shacham_waters_private.cxx:638-702 per file; one prime per Swizzle,
:596-624)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError
from test_encode_mixed import BEATS, P61, P256, P1024, EncodeMixedLib, _blob, _w


class CxxEncodeMixedLib(EncodeMixedLib):
    """EncodeMixedLib over the oracle's cxx encode, with the State's AES."""
    oracle_fn = "cxx_encode"

    def hb_aes_cfb128(self, key, klen, iv, data, out, n, encrypt):
        pad = (bytes(key[:klen]) + bytes(iv[:16])) * (n // 16 + 1)
        ctypes.memmove(out, bytes(a ^ b for a, b in zip(bytes(data[:n]), pad)), n)
        return 0

    def hb_encode(self, h, pb, plen, sectors, fk, ak, klen, block_base, data, length, nblocks, tags, flags, tries):
        from heartbeat_amd import _native
        assert flags & _native.HB_PRF_CXX
        return EncodeMixedLib.hb_encode(self, h, pb, plen, sectors, fk, ak, klen, block_base, data, length, nblocks, tags,
                                        flags, tries)

    def hb_cxx_encode_mixed(self, h, descs, n, flags, tries):
        return self._mixed(descs, n, flags, tries)

    # the PySwizzle mixed call must not be what the cxx Swizzle reaches
    def hb_encode_mixed(self, *a):
        raise AssertionError("the cxx Swizzle called hb_encode_mixed")


@pytest.fixture
def swz():
    return importlib.import_module("heartbeat_amd.Swizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = CxxEncodeMixedLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


def _items(swz, n):
    """n (beat, file), beats interleaved."""
    beats = [swz.Swizzle(sectors=S, prime=p) for p, S in BEATS]
    return [(beats[k % 3], io.BytesIO(_blob(k))) for k in range(n)]


def _check_results(oracle, swz, items, blobs, res):
    for (beat, f), blob, (tag, state) in zip(items, blobs, res):
        assert isinstance(tag, swz.Tag) and isinstance(state, swz.State) and state.encrypted
        state = swz.State.fromdict(state.todict())              # as stored: no keys in the clear
        assert state.f_key == b""
        state.decrypt(beat.k_enc, beat.k_mac)
        assert len(state.f_key) == 32 and len(state.alpha_key) == 32
        C = beat.sectorsize * beat.sectors
        assert state.n == len(blob) // C + 1 == len(tag)
        assert tag.sigma == oracle.cxx_encode(beat.prime, beat.sectors, state.f_key, state.alpha_key, blob)


def test_encode_mixed_three_beats_interleaved(lib, oracle, swz):
    items = _items(swz, 8)
    blobs = [f.getvalue() for _, f in items]
    res = swz.Swizzle.encode_mixed(items)
    assert lib.single == 0
    (flags, seen), = lib.mixed                                  # one call, no single encode
    assert flags == 0
    assert seen == [(b.prime, b.sectors, 32, len(blob)) for (b, f), blob in zip(items, blobs)]
    assert len({s[0] for s in seen}) == 3
    _check_results(oracle, swz, items, blobs, res)
    keys = {s.f_key for _, s in res} | {s.alpha_key for _, s in res}
    assert len(keys) == 16                                      # fresh keys per file
    assert all(f.tell() == len(blob) for (_, f), blob in zip(items, blobs))


def test_states_decrypt_under_their_own_beat_only(lib, swz):
    items = _items(swz, 6)
    res = swz.Swizzle.encode_mixed(items)
    for k, ((beat, _), (tag, state)) in enumerate(zip(items, res)):
        other = items[(k + 1) % 6][0]
        stored = swz.State.fromdict(state.todict())
        stored.decrypt(other.k_enc, other.k_mac)                # a bad signature leaves the state as it is
        assert stored.f_key == b"" and stored.alpha_key == b""
        stored.decrypt(beat.k_enc, beat.k_mac)
        assert stored.f_key == state.f_key and stored.alpha_key == state.alpha_key and len(stored.f_key) == 32


def test_files_encoded_from_mid_position_and_left_at_eof(lib, oracle, swz, tmp_path):
    items = _items(swz, 5)
    blobs = [f.getvalue() for _, f in items]
    path = tmp_path / "real.bin"
    path.write_bytes(blobs[3])
    with open(str(path), "rb") as fh:
        items[3] = (items[3][0], fh)
        skips = [0, 0, 40, 300, 1]
        for (_, f), k in zip(items, skips):
            f.seek(k)
        res = swz.Swizzle.encode_mixed(items)
        assert [f.tell() for _, f in items] == [len(b) for b in blobs]      # left at EOF
        _check_results(oracle, swz, items, [b[k:] for b, k in zip(blobs, skips)], res)


class Unreadable(object):
    def read(self, *a):
        raise IOError("no such medium")

    def tell(self):
        return 0


def test_error_order_of_a_loop(lib, swz):
    """A beat without sectors at item 2 and one with a 7-bit prime at item 3:
    item 2's error, as a loop's; nothing is called and no file is read."""
    def build():
        items = _items(swz, 5)
        items[2] = (swz.Swizzle(sectors=0, prime=P256), items[2][1])
        items[3] = (swz.Swizzle(sectors=3, prime=127), items[3][1])
        return items
    items = build()
    with pytest.raises(HeartbeatError) as e:
        swz.Swizzle.encode_mixed(items)
    with pytest.raises(HeartbeatError) as e1:
        [b.encode(f) for b, f in build()]
    assert str(e.value) == str(e1.value) == "sectors must be positive"
    assert lib.mixed == []
    assert [f.tell() for _, f in items] == [0] * 5
    # a file that cannot be read: every file is opened first, the files before
    # it are left at EOF as the loop leaves them, and nothing is called
    items = _items(swz, 3)
    items[1] = (items[1][0], Unreadable())
    with pytest.raises(IOError):
        swz.Swizzle.encode_mixed(items)
    assert lib.mixed == []
    assert items[0][1].tell() == len(items[0][1].getvalue()) and items[2][1].tell() == 0


def test_below_threshold_goes_through_encode(lib, oracle, swz, monkeypatch):
    monkeypatch.setattr(swz, "CXX_ENCODE_MIXED_MIN", 3)
    items = _items(swz, 2)
    res = swz.Swizzle.encode_mixed(items)
    assert lib.single == 2 and lib.mixed == []
    _check_results(oracle, swz, items, [_blob(0), _blob(1)], res)
    items = _items(swz, 3)
    res = swz.Swizzle.encode_mixed(items)
    assert lib.single == 2 and len(lib.mixed) == 1
    _check_results(oracle, swz, items, [_blob(k) for k in range(3)], res)


def test_empty_list_makes_no_library_call(lib, swz):
    assert swz.Swizzle.encode_mixed([]) == []
    assert swz.encode_files_mixed([]) == []
    assert lib.mixed == [] and lib.single == 0


def test_encode_files_mixed_explicit_keys(lib, oracle, swz):
    blobs = [_blob(2), _blob(3), b""]
    items = [(P256, 16, b"f" * 16, b"a" * 16, io.BytesIO(blobs[0])),
             (P61, 3, b"g" * 24, b"b" * 24, blobs[1]),
             (P1024, 10, b"h" * 32, b"c" * 32, io.BytesIO(blobs[2]))]
    res = swz.encode_files_mixed(items)
    (flags, seen), = lib.mixed
    assert [s[:3] for s in seen] == [(P256, 16, 16), (P61, 3, 24), (P1024, 10, 32)]
    for (p, S, fk, ak, _), blob, (tag, nblocks) in zip(items, blobs, res):
        assert tag.sigma == oracle.cxx_encode(p, S, fk, ak, blob) and nblocks == len(tag)
        assert tag._width == _w(p)
    with pytest.raises(HeartbeatError):
        swz.encode_files_mixed([(P256, 0, b"f" * 16, b"a" * 16, b"x")])
    assert len(lib.mixed) == 1


def test_heartbeat_is_the_cxx_swizzle():
    import heartbeat
    assert heartbeat.Heartbeat.encode_mixed is importlib.import_module("heartbeat_amd.Swizzle").Swizzle.encode_mixed
