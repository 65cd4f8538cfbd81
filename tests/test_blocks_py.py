"""CPU tests of the listed-block update's Python layer (PySwizzle.encode_blocks,
patch_tag, update, update_file, update_many) over an oracle-backed stand-in for
hb_encode_blocks_many (tests/blocks_fake.py) -- no GPU.

Reference: the body of heartbeat/PySwizzle/PySwizzle.py:296-309 for chosen i,
i.e. oracle.encode(..., block_base=i, nblocks=1), and oracle.encode of the
whole new file under the state's keys."""
import copy
import importlib
import io

import pytest

import blocks_fake
from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S
KEY = b"K" * 32
FK, AK = b"\x11" * 32, b"\x22" * 32


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def fake(monkeypatch):
    return blocks_fake.install(monkeypatch)


def _data(n, salt=0):
    return bytes((i * 7 + salt + (i >> 8)) & 0xff for i in range(n))


def _tagged(pys, oracle, data, raw=True):
    """(beat, tag, state) of `data` under FK / AK, the tag as encode leaves it
    (raw image) or as fromdict does (list)."""
    beat = pys.PySwizzle(S, KEY, P256)
    sigma = oracle.encode(P256, S, FK, AK, data)
    if raw:
        tag = pys.Tag._from_raw(memoryview(b"".join(s.to_bytes(32, "big") for s in sigma)), 32)
    else:
        tag = pys.Tag.fromdict({"sigma": list(sigma)})
    state = pys.State(FK, AK, len(sigma))
    state.encrypt(KEY)
    return beat, tag, state


def _blocks_of(data, indices):
    return [(i, data[i * C:(i + 1) * C]) for i in indices]


def _snapshot(tag, state):
    return (list(tag.sigma) if tag._sigma is not None else bytes(tag._raw), tag._sigma is None,
            dict(state.__dict__))


def _same(tag, state, snap):
    return _snapshot(tag, state) == snap


def _keys_of(beat, state):
    st = copy.copy(state)
    st.decrypt(beat.key)
    return bytes(st.f_key), bytes(st.alpha_key), st.chunks


# ------------------------------------------------------------------ encode_blocks
def test_encode_blocks_sorts_and_matches_oracle(fake, oracle, pys):
    data = _data(5 * C + 9)
    beat, tag, state = _tagged(pys, oracle, data)
    snap = _snapshot(tag, state)
    idx, patch = beat.encode_blocks(state, _blocks_of(data, [5, 0, 3]))
    assert idx == [0, 3, 5]
    assert fake.block_calls == [(1, [3])]
    want = oracle.encode(P256, S, FK, AK, data)
    assert patch.sigma == [want[0], want[3], want[5]]
    assert patch._width == 32
    assert _same(tag, state, snap) and state.encrypted          # the argument keeps its ciphertext
    # an index the file never had: the value is F(i) + MAC all the same
    idx, patch = beat.encode_blocks(state, [(2 ** 64 - 1, b"xyz")])
    assert patch.sigma == oracle.encode(P256, S, FK, AK, b"xyz", block_base=2 ** 64 - 1, nblocks=1)


def test_encode_blocks_errors(fake, oracle, pys):
    data = _data(3 * C)
    beat, tag, state = _tagged(pys, oracle, data)
    with pytest.raises(HeartbeatError, match="block index 1 is listed twice"):
        beat.encode_blocks(state, [(1, b"a" * C), (0, b"b" * C), (1, b"c" * C)])
    with pytest.raises(HeartbeatError, match="block 0 has 5 bytes, not 128"):
        beat.encode_blocks(state, [(0, b"short"), (1, b"a" * C)])     # only the highest index may be short
    with pytest.raises(HeartbeatError, match="block 2 has 129 bytes"):
        beat.encode_blocks(state, [(2, b"a" * (C + 1))])
    with pytest.raises(HeartbeatError, match="outside"):
        beat.encode_blocks(state, [(-1, b"")])
    with pytest.raises(HeartbeatError, match="outside"):
        beat.encode_blocks(state, [(2 ** 64, b"")])
    bad = copy.copy(state)
    bad.chunks += 1
    with pytest.raises(HeartbeatError, match="Signature invalid"):
        beat.encode_blocks(bad, [(0, b"a" * C)])
    assert fake.block_calls == []                               # nothing reached the library


# ------------------------------------------------------------------ patch_tag
@pytest.mark.parametrize("raw", [True, False])
def test_patch_tag_replaces_grows_and_shrinks(fake, oracle, pys, raw):
    data = _data(4 * C + 1)
    _, tag, _ = _tagged(pys, oracle, data, raw=raw)
    before = list(oracle.encode(P256, S, FK, AK, data))
    assert len(tag) == 5
    out = pys.PySwizzle.patch_tag(tag, [3, 1], [7, 9])
    # raw stays raw, a list stays a list (looked at before .sigma materialises the list)
    assert (out._sigma is None and out._width == 32) if raw else (out._raw is None and out._sigma is not None)
    if raw:
        assert bytes(out.raw(P256))[32:64] == (9).to_bytes(32, "big") and len(bytes(out.raw(P256))) == 5 * 32
    assert out.sigma == [before[0], 9, before[2], 7, before[4]] and len(out) == 5
    assert tag.sigma == before                                  # the argument is not modified
    _, tag, _ = _tagged(pys, oracle, data, raw=raw)
    grown = pys.PySwizzle.patch_tag(tag, [4, 6, 5], [1, 3, 2], nblocks=7)
    assert grown.sigma == before[:4] + [1, 2, 3]
    with pytest.raises(HeartbeatError, match="block 5 is added but not listed"):
        pys.PySwizzle.patch_tag(tag, [4, 6], [1, 3], nblocks=7)
    shrunk = pys.PySwizzle.patch_tag(tag, [1], [5], nblocks=2)
    assert shrunk.sigma == [before[0], 5]
    with pytest.raises(HeartbeatError, match="block index 2 is outside the tag's 2 blocks"):
        pys.PySwizzle.patch_tag(tag, [2], [5], nblocks=2)
    with pytest.raises(HeartbeatError, match="2 indices for 1 values"):
        pys.PySwizzle.patch_tag(tag, [0, 1], [5])
    # values as a Tag (what encode_blocks returns)
    vals = pys.Tag._from_raw(memoryview((11).to_bytes(32, "big") + (12).to_bytes(32, "big")), 32)
    out = pys.PySwizzle.patch_tag(tag, [0, 2], vals)
    assert out.sigma[0] == 11 and out.sigma[2] == 12 and out.sigma[1] == before[1]
    if raw:
        with pytest.raises(HeartbeatError, match="does not fit"):
            pys.PySwizzle.patch_tag(tag, [0], [1 << 256])


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("raw", [True, False])
def test_update_in_place_tail_append_truncate(fake, oracle, pys, raw):
    old = _data(5 * C + 40)
    beat, tag, state = _tagged(pys, oracle, old, raw=raw)
    snap = _snapshot(tag, state)
    old_sigma = list(oracle.encode(P256, S, FK, AK, old))

    def check(new, blocks, length):
        t2, s2 = beat.update(tag, state, blocks, length)
        assert (t2._sigma is None) == raw                       # looked at before .sigma materialises the list
        assert t2.sigma == oracle.encode(P256, S, FK, AK, new)
        fk, ak, chunks = _keys_of(beat, s2)
        assert (fk, ak) == (FK, AK) and chunks == len(new) // C + 1      # the same two PRF keys
        assert s2.encrypted and s2.iv != state.iv and s2.hmac == s2.get_hmac(KEY)
        assert _same(tag, state, snap)
        return t2, s2

    # in-place edit of blocks 1 and 3
    new = bytearray(old)
    new[C + 5] ^= 0xff
    new[3 * C:3 * C + 3] = b"abc"
    new = bytes(new)
    t2, _ = check(new, _blocks_of(new, [3, 1]), None)
    assert [i for i in range(6) if t2.sigma[i] != old_sigma[i]] == [1, 3]
    check(new, _blocks_of(new, [3, 1]), len(new))               # the same with the length given
    # the tail alone, shorter and longer within its block
    for n in (5 * C, 5 * C + 1, 5 * C + 127):
        new = old[:5 * C] + _data(n - 5 * C, 3)
        check(new, [(5, new[5 * C:])], None)
        check(new, [(5, new[5 * C:])], n)
    # append across a block boundary: the old last block with its new bytes, and the new blocks
    new = old + _data(2 * C, 9)
    check(new, _blocks_of(new, [5, 6, 7]), len(new))
    # append to a multiple of C: the empty last block is listed too
    new = old + _data(C - 40, 9)
    assert len(new) == 6 * C
    check(new, _blocks_of(new, [5, 6]), len(new))
    # truncate: the new last block
    new = old[:2 * C + 17]
    t2, s2 = check(new, [(2, new[2 * C:])], len(new))
    assert len(t2) == 3
    new = b""
    check(new, [(0, b"")], 0)


def test_update_errors_before_any_call(fake, oracle, pys):
    old = _data(5 * C + 40)                                     # n = 6
    beat, tag, state = _tagged(pys, oracle, old)
    full = b"f" * C

    def fails(msg, blocks, length=None):
        with pytest.raises(HeartbeatError, match=msg):
            beat.update(tag, state, blocks, length)

    fails("block index 6 is outside the file's 6 blocks", [(1, full), (6, b""), (9, b"")])
    fails("block index -1 is outside", [(-1, full)])
    fails("block index 1 is listed twice", [(1, full), (2, full), (1, full)])
    fails("block index 3 is outside the file's 3 blocks", [(3, full)], 2 * C + 1)
    # growing from 6 to 8 blocks: 5, 6 and 7 must be listed
    fails("block 5 must be listed when the file goes from 6 to 8 blocks", [(6, full), (7, b"x")], 7 * C + 1)
    fails("block 6 must be listed when the file goes from 6 to 8 blocks", [(5, full), (7, b"x")], 7 * C + 1)
    # shrinking to 3 blocks: the new last block
    fails("block 2 must be listed when the file goes from 6 to 3 blocks", [(0, full)], 2 * C + 1)
    # lengths
    fails("block 1 has 127 bytes, not 128", [(1, full[:-1])])
    fails("block 5 has 40 bytes, not 128", [(5, b"y" * 40), (6, full), (7, b"x")], 7 * C + 1)
    fails("the last block 7 has 2 bytes, not 1", [(5, full), (6, full), (7, b"xx")], 7 * C + 1)
    fails("the last block 5 has 128 bytes, not fewer than 128", [(5, full)])
    fails("the last block 5 has 3 bytes, not 40", [(5, b"abc")], 5 * C + 40)
    fails("length must not be negative", [(0, full)], -1)
    bad = copy.copy(state)
    bad.hmac = b"\0" * 32
    with pytest.raises(HeartbeatError, match="Signature invalid"):
        beat.update(tag, bad, [(1, full)])
    assert fake.block_calls == []


# ------------------------------------------------------------------ update_file
def test_file_blocks_from_byte_ranges(fake, oracle, pys):
    old = _data(5 * C + 40)
    beat, tag, state = _tagged(pys, oracle, old)
    from heartbeat_amd._filebuf import FileBuffer

    def picked(new, changed):
        fb = FileBuffer(io.BytesIO(new), from_start=True)
        blocks, length = beat._file_blocks(state, fb, changed)
        assert length == len(new)
        assert all(d == new[i * C:(i + 1) * C] for i, d in blocks)
        return [i for i, _ in blocks]

    assert picked(old, []) == []
    assert picked(old, [(0, 1)]) == [0]
    assert picked(old, [(C - 1, 1)]) == [0] and picked(old, [(C - 1, 2)]) == [0, 1] and picked(old, [(C, 1)]) == [1]
    assert picked(old, [(C, 0)]) == []                          # an empty range touches nothing
    assert picked(old, [(3 * C + 5, 2 * C), (10, 1), (C + 1, 1)]) == [0, 1, 3, 4, 5]
    assert picked(old, [(5 * C + 39, 1)]) == [5]
    grown = old + _data(C, 1)                                   # 6 -> 7 blocks: 5 and 6 by the length rule
    assert picked(grown, []) == [5, 6]
    assert picked(grown, [(2, 2)]) == [0, 5, 6]
    assert picked(old[:C], []) == [1]                           # 6 -> 2 blocks: min(n, n') - 1 = n' - 1 = 1, now empty
    assert picked(old[:C + 9], [(3, 1)]) == [0, 1]
    with pytest.raises(HeartbeatError, match=r"range \(700, 1\) is outside the file's 680 bytes"):
        picked(old, [(len(old) + 20, 1)])
    with pytest.raises(HeartbeatError, match="outside"):
        picked(old, [(-1, 2)])


def test_update_file_equals_update_and_restores_position(fake, oracle, pys, tmp_path):
    old = _data(5 * C + 40)
    beat, tag, state = _tagged(pys, oracle, old)
    new = bytearray(old + _data(C + 3, 5))
    new[2 * C + 1] ^= 1
    new = bytes(new)
    path = tmp_path / "new.bin"
    path.write_bytes(new)
    for file in (io.BytesIO(new), open(str(path), "rb")):
        try:
            file.seek(77)
            t2, s2 = beat.update_file(tag, state, file, [(2 * C + 1, 1), (len(old), C + 3)])
            assert file.tell() == 77
        finally:
            file.close()
        assert t2.sigma == oracle.encode(P256, S, FK, AK, new)
        assert _keys_of(beat, s2) == (FK, AK, 7)
        t3, _ = beat.update(tag, state, _blocks_of(new, [2, 5, 6]), len(new))
        assert t3.sigma == t2.sigma
    assert fake.block_calls == [(1, [3])] * 4


# ------------------------------------------------------------------ update_many
def test_update_many_equals_loop(fake, oracle, pys, monkeypatch):
    beat = pys.PySwizzle(S, KEY, P256)
    items, news = [], []
    for k in range(4):
        old = _data((k + 1) * C + 10 * k, k)
        sigma = oracle.encode(P256, S, bytes([k + 1]) * 32, bytes([k + 9]) * 32, old)
        tag = pys.Tag._from_raw(memoryview(b"".join(s.to_bytes(32, "big") for s in sigma)), 32)
        state = pys.State(bytes([k + 1]) * 32, bytes([k + 9]) * 32, len(sigma))
        state.encrypt(KEY)
        if k == 2:                                              # an item without any block
            items.append((tag, state, iter([]), None))
            news.append(old)
            continue
        new = bytes(b ^ 0x55 for b in old[:C]) + old[C:] + (_data(C, 40 + k) if k == 3 else b"")
        n_old, n_new = len(old) // C + 1, len(new) // C + 1
        idx = sorted({0} | (set(range(n_old - 1, n_new)) if n_new != n_old else set()))
        items.append((tag, state, iter(_blocks_of(new, idx)), len(new)))     # an iterator is read once
        news.append(new)
    res = beat.update_many(items)
    assert fake.block_calls == [(4, [1, 1, 0, 3])]              # one call for the batch
    for k, ((t2, s2), new) in enumerate(zip(res, news)):
        assert t2.sigma == oracle.encode(P256, S, bytes([k + 1]) * 32, bytes([k + 9]) * 32, new)
        assert _keys_of(beat, s2) == (bytes([k + 1]) * 32, bytes([k + 9]) * 32, len(new) // C + 1)
        assert s2.encrypted
    # below UPDATE_MANY_MIN: the loop
    monkeypatch.setattr(pys, "UPDATE_MANY_MIN", 9)
    fake.block_calls[:] = []
    tag, state = items[0][0], items[0][1]
    again = beat.update_many([(tag, state, _blocks_of(news[0], [0]), len(news[0]))] * 2)
    assert fake.block_calls == [(1, [1]), (1, [1])]
    assert again[0][0].sigma == res[0][0].sigma
    assert beat.update_many([]) == []


def test_update_many_raises_the_loops_first_error(fake, oracle, pys):
    old = _data(3 * C + 1)
    beat, tag, state = _tagged(pys, oracle, old)
    good = (tag, state, [(0, old[:C])], None)
    bad_len = (tag, state, [(1, b"short")], None)
    bad_idx = (tag, state, [(4, b"")], None)
    with pytest.raises(HeartbeatError, match="block 1 has 5 bytes, not 128"):
        beat.update_many([good, bad_len, bad_idx])
    with pytest.raises(HeartbeatError, match="block index 4 is outside the file's 4 blocks"):
        beat.update_many([good, bad_idx, bad_len])
    assert fake.block_calls == []                               # before any GPU work
