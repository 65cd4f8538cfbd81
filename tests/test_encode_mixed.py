"""CPU tests of the mixed-owner encode's Python layer (heartbeat_amd._many:
encode_files_mixed; PySwizzle.encode_mixed and the module-level
encode_files_mixed) over a small stand-in for libhbswizzle.so whose
hb_encode_mixed reads each descriptor's nine raw words and answers with the CPU
oracle -- no GPU.

Three beats -- a 256-bit prime with S = 16, a 1024-bit one with S = 10, a
61-bit one with S = 3 -- interleaved in one call.

Reference: a loop of b.encode(file) over the beats of many owners
(PySwizzle.py:279-311 per file, one prime per PySwizzle instance, :250-251)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
# odd numbers of the right bit lengths: the oracle and the stand-in need no primality
P1024 = (1 << 1023) | int.from_bytes(bytes(range(1, 128)), "big") | 1
P61 = (1 << 60) | 0x123456789abcdf
BEATS = [(P256, 16), (P1024, 10), (P61, 3)]
KEYS = [b"A" * 32, b"B" * 32, b"C" * 32]


def _w(p):
    return (p.bit_length() + 7) // 8


class EncodeMixedLib(object):
    """A context, the single hb_encode and hb_encode_mixed over the oracle.
    `single` counts hb_encode calls, `mixed` records every mixed call's
    descriptors as they carried them."""
    oracle_fn = "encode"

    def __init__(self):
        self.single = 0
        self.mixed = []

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

    def _tags(self, p, sectors, fk, ak, data):
        from oracle import oracle as O
        return b"".join(t.to_bytes(_w(p), "big") for t in getattr(O, self.oracle_fn)(p, sectors, fk, ak, data))

    def hb_encode(self, h, pb, plen, sectors, fk, ak, klen, block_base, data, length, nblocks, tags, flags, tries):
        assert block_base == 0
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.single += 1
        addr = data if isinstance(data, int) else getattr(data, "value", None)
        blob = ctypes.string_at(addr, int(length)) if length else b""
        raw = self._tags(p, sectors, bytes(fk[:klen]), bytes(ak[:klen]), blob)
        assert len(raw) == nblocks * _w(p)
        ctypes.memmove(tags if isinstance(tags, int) else tags.value, raw, len(raw))
        return 0

    def _mixed(self, descs, n, flags, tries):
        seen, total = [], 0
        for i in range(n):
            # p_be, p_len, sectors, key_len, then hb_file_desc's five words: f_key, alpha_key, data, len, tags
            x = (ctypes.c_uint64 * 9).from_address(ctypes.addressof(descs[i]))
            p = int.from_bytes(ctypes.string_at(x[0], x[1]), "big")
            S, klen = int(x[2]), int(x[3])
            seen.append((p, S, klen, int(x[7])))
            data = ctypes.string_at(x[6], x[7]) if x[7] else b""
            raw = self._tags(p, S, ctypes.string_at(x[4], klen), ctypes.string_at(x[5], klen), data)
            ctypes.memmove(x[8], raw, len(raw))
            total += len(raw) // _w(p)
        self.mixed.append((int(flags), seen))
        tries._obj.value = total
        return 0

    def hb_encode_mixed(self, h, descs, n, flags, tries):
        return self._mixed(descs, n, flags, tries)

    def hb_cxx_encode_mixed(self, *a):
        raise AssertionError("PySwizzle called hb_cxx_encode_mixed")


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = EncodeMixedLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])

    def xor_cfb8(key, iv, data, encrypt):                      # a reversible stand-in for hb_aes_cfb8
        pad = (bytes(key) + bytes(iv)) * (len(data) // 16 + 1)
        return bytes(a ^ b for a, b in zip(bytes(data), pad))

    monkeypatch.setattr(_native, "aes_cfb8", xor_cfb8)
    return fake


def _beats(pys):
    return [pys.PySwizzle(S, key, p) for (p, S), key in zip(BEATS, KEYS)]


def _blob(k):
    """File k: empty, shorter than a sector, and a few blocks long, in turn."""
    return bytes((7 * k + i) & 0xff for i in range([0, 5, 150, 777, 1300][k % 5] + 3 * k))


def _items(pys, n):
    """n (beat, file), beats interleaved."""
    beats = _beats(pys)
    return [(beats[k % 3], io.BytesIO(_blob(k))) for k in range(n)]


def _check_results(oracle, items, blobs, res, pys):
    for (beat, f), blob, (tag, state) in zip(items, blobs, res):
        assert isinstance(tag, pys.Tag) and isinstance(state, pys.State) and state.encrypted
        state.decrypt(beat.key)
        C = (int(beat.prime).bit_length() // 8) * beat.sectors
        assert state.chunks == len(blob) // C + 1 == len(tag)
        assert tag.sigma == oracle.encode(beat.prime, beat.sectors, state.f_key, state.alpha_key, blob)
        assert tag._width == _w(beat.prime)


def test_encode_mixed_three_beats_interleaved(lib, oracle, pys):
    items = _items(pys, 8)
    blobs = [f.getvalue() for _, f in items]
    res = pys.PySwizzle.encode_mixed(items)
    assert lib.single == 0
    (flags, seen), = lib.mixed                                  # one call, no single encode
    assert flags == 0
    # every descriptor carries its own item's prime, S, key length and file length
    assert seen == [(int(b.prime), int(b.sectors), 32, len(blob)) for (b, f), blob in zip(items, blobs)]
    assert len({s[0] for s in seen}) == 3
    _check_results(oracle, items, blobs, res, pys)
    keys = {s.f_key for _, s in res} | {s.alpha_key for _, s in res}
    assert len(keys) == 16                                      # fresh keys per file
    assert all(f.tell() == len(blob) for (_, f), blob in zip(items, blobs))
    # any iterable
    res = pys.PySwizzle.encode_mixed(iter(_items(pys, 4)))
    assert len(res) == 4 and len(lib.mixed) == 2


def test_states_decrypt_under_their_own_beat_only(lib, oracle, pys):
    items = _items(pys, 6)
    res = pys.PySwizzle.encode_mixed(items)
    for k, ((beat, _), (tag, state)) in enumerate(zip(items, res)):
        other = items[(k + 1) % 6][0]
        assert other.key != beat.key
        with pytest.raises(HeartbeatError) as e:
            pys.State.fromdict(state.todict()).decrypt(other.key)
        assert str(e.value) == "Signature invalid on state."
        state.decrypt(beat.key)
        assert not state.encrypted


def test_files_encoded_from_mid_position_and_left_at_eof(lib, oracle, pys, tmp_path):
    items = _items(pys, 5)
    blobs = [f.getvalue() for _, f in items]
    path = tmp_path / "real.bin"
    path.write_bytes(blobs[3])
    with open(str(path), "rb") as fh:
        items[3] = (items[3][0], fh)
        skips = [0, 0, 40, 300, 1]
        for (_, f), k in zip(items, skips):
            f.seek(k)
        res = pys.PySwizzle.encode_mixed(items)
        assert [f.tell() for _, f in items] == [len(b) for b in blobs]      # left at EOF
        _check_results(oracle, items, [b[k:] for b, k in zip(blobs, skips)], res, pys)
        (flags, seen), = lib.mixed
        assert [s[3] for s in seen] == [len(b) - k for b, k in zip(blobs, skips)]


def test_error_order_of_a_loop(lib, pys):
    """A beat without sectors at item 2 and one with a 7-bit prime at item 3:
    item 2's error, as a loop's; nothing is called and no file is read."""
    items = _items(pys, 5)
    items[2] = (pys.PySwizzle(0, b"K" * 32, P256), items[2][1])
    items[3] = (pys.PySwizzle(3, b"K" * 32, 127), items[3][1])
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.encode_mixed(items)
    items2 = _items(pys, 5)
    items2[2] = (pys.PySwizzle(0, b"K" * 32, P256), items2[2][1])
    items2[3] = (pys.PySwizzle(3, b"K" * 32, 127), items2[3][1])
    with pytest.raises(HeartbeatError) as e1:
        [b.encode(f) for b, f in items2]
    assert str(e.value) == str(e1.value) == "sectors must be positive"
    assert lib.mixed == []
    assert [f.tell() for _, f in items] == [0] * 5
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.encode_mixed(items[3:])
    assert "prime must be at least 2^8" in str(e.value)
    assert lib.mixed == []


def test_below_threshold_goes_through_encode(lib, oracle, pys, monkeypatch):
    monkeypatch.setattr(pys, "ENCODE_MIXED_MIN", 3)
    items = _items(pys, 2)
    blobs = [f.getvalue() for _, f in items]
    res = pys.PySwizzle.encode_mixed(items)
    assert lib.single == 2 and lib.mixed == []
    _check_results(oracle, items, blobs, res, pys)
    items = _items(pys, 3)
    res = pys.PySwizzle.encode_mixed(items)
    assert lib.single == 2 and len(lib.mixed) == 1
    _check_results(oracle, items, [_blob(k) for k in range(3)], res, pys)


def test_empty_list_makes_no_library_call(lib, pys):
    from heartbeat_amd import _many
    assert pys.PySwizzle.encode_mixed([]) == []
    assert pys.encode_files_mixed([]) == []
    assert _many.encode_files_mixed([], "hb_encode_mixed", pys.Tag, False) == []
    assert lib.mixed == [] and lib.single == 0


def test_encode_files_mixed_explicit_keys(lib, oracle, pys):
    blobs = [_blob(2), _blob(3), b""]
    items = [(P256, 16, b"f" * 16, b"a" * 16, io.BytesIO(blobs[0])),
             (P61, 3, b"g" * 24, b"b" * 24, blobs[1]),
             (P1024, 10, b"h" * 32, b"c" * 32, io.BytesIO(blobs[2]))]
    res = pys.encode_files_mixed(items)
    (flags, seen), = lib.mixed
    assert [s[:3] for s in seen] == [(P256, 16, 16), (P61, 3, 24), (P1024, 10, 32)]
    for (p, S, fk, ak, _), blob, (tag, nblocks) in zip(items, blobs, res):
        assert tag.sigma == oracle.encode(p, S, fk, ak, blob) and nblocks == len(tag)
    n = len(lib.mixed)
    with pytest.raises(HeartbeatError):
        pys.encode_files_mixed([(P256, 0, b"f" * 16, b"a" * 16, b"x")])
    with pytest.raises(HeartbeatError):
        pys.encode_files_mixed([(127, 3, b"f" * 16, b"a" * 16, b"x")])
    with pytest.raises(HeartbeatError):
        pys.encode_files_mixed([(P256, 4, b"f" * 16, b"a" * 32, b"x")])
    assert len(lib.mixed) == n


def test_descriptor_layout():
    """hb_encode_mixed_desc (hbswizzle.h): nine 8-byte words, hb_file_desc's last."""
    from heartbeat_amd import _native
    D = _native.EncodeMixedDesc
    names = ["p_be", "p_len", "sectors", "key_len"] + [f[0] for f in _native.FileDesc._fields_]
    assert ctypes.sizeof(D) == 72 and [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == list(range(0, 72, 8))
    sig = {name: args for name, _, args in _native.SIGNATURES}
    for name in ("hb_encode_mixed", "hb_cxx_encode_mixed"):
        assert sig[name][1] == ctypes.POINTER(D) and len(sig[name]) == 5
