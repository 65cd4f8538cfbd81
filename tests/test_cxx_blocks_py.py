"""CPU tests of the cxx Swizzle's listed-block update (heartbeat.Heartbeat:
encode_blocks, patch_tag, update, update_file, update_many) over an
oracle-backed stand-in for hb_cxx_encode_blocks_many (tests/cxx_blocks_fake.py)
-- no GPU.

Reference: the body of cxx/shacham_waters_private.cxx:674-694 for chosen
chunk_id, i.e. oracle.cxx_encode(..., block_base=i, nblocks=1), and
oracle.cxx_encode of the whole new file under the state's keys."""
import io

import pytest

import cxx_blocks_fake
from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S
FK, AK = b"\x11" * 32, b"\x22" * 32


@pytest.fixture
def sw():
    import heartbeat_amd.Swizzle as mod
    return mod


@pytest.fixture
def fake(monkeypatch):
    return cxx_blocks_fake.install(monkeypatch)


def _data(n, salt=0):
    return bytes((i * 7 + salt + (i >> 8)) & 0xff for i in range(n))


def _state(sw, beat, fk, ak, n):
    st = sw.State()
    st.n, st.f_key, st.alpha_key = n, fk, ak
    st.encrypt(beat.k_enc, beat.k_mac)
    return st


def _tag(sw, sigma, raw=True):
    tag = sw.Tag._from_raw(memoryview(b"".join(s.to_bytes(32, "big") for s in sigma)), 32)
    if not raw:                                                 # as fromdict leaves it: a list
        tag = sw.Tag.fromdict(tag.todict())
        assert tag._raw is None
    return tag


def _tagged(sw, oracle, data, raw=True):
    """(beat, tag, state) of `data` under FK / AK, the tag as encode leaves it
    (raw image) or as fromdict does (list)."""
    beat = sw.Swizzle(1.0, S, True, P256)
    sigma = oracle.cxx_encode(P256, S, FK, AK, data)
    return beat, _tag(sw, sigma, raw), _state(sw, beat, FK, AK, len(sigma))


def _blocks_of(data, indices):
    return [(i, data[i * C:(i + 1) * C]) for i in indices]


def _snapshot(tag, state):
    return (list(tag._sigma) if tag._sigma is not None else bytes(tag._raw), tag._sigma is None, dict(state.__dict__))


def _keys_of(beat, state):
    s = state._copy()
    assert s._check_sig_and_decrypt(beat.k_enc, beat.k_mac)
    return bytes(s.f_key), bytes(s.alpha_key), s.n


def _forged(state):
    bad = state._copy()
    bad._raw = bad._raw[:-1] + bytes([bad._raw[-1] ^ 1])        # one bit of the MAC
    return bad


# ------------------------------------------------------------------ encode_blocks
def test_encode_blocks_sorts_and_matches_oracle(fake, oracle, sw):
    data = _data(5 * C + 9)
    beat, tag, state = _tagged(sw, oracle, data)
    snap = _snapshot(tag, state)
    blocks = _blocks_of(data, [5, 0, 3])
    idx, patch = beat.encode_blocks(state, iter(blocks))
    assert idx == [0, 3, 5]
    assert fake.block_calls == [(1, [3])]
    want = oracle.cxx_encode(P256, S, FK, AK, data)
    assert patch.sigma == [want[0], want[3], want[5]]
    assert patch._width == 32
    assert _snapshot(tag, state) == snap and blocks == _blocks_of(data, [5, 0, 3])   # the arguments are as they were
    # the highest index the prf takes, and an empty block: f(index) unreduced
    idx, patch = beat.encode_blocks(state, [(2 ** 32 - 1, b"")])
    assert patch.sigma == [oracle.cxx_prf_eval(FK, P256, 2 ** 32 - 1)[0]]


def test_encode_blocks_errors(fake, oracle, sw):
    data = _data(3 * C)
    beat, tag, state = _tagged(sw, oracle, data)
    with pytest.raises(HeartbeatError, match="block index 1 is listed twice"):
        beat.encode_blocks(state, [(1, b"a" * C), (0, b"b" * C), (1, b"c" * C)])
    with pytest.raises(HeartbeatError, match="block 0 has 5 bytes, not 128"):
        beat.encode_blocks(state, [(0, b"short"), (1, b"a" * C)])     # only the highest index may be short
    with pytest.raises(HeartbeatError, match="block 2 has 129 bytes"):
        beat.encode_blocks(state, [(2, b"a" * (C + 1))])
    with pytest.raises(HeartbeatError, match=r"block index -1 is outside \[0, 2\^32\)"):
        beat.encode_blocks(state, [(-1, b"")])
    with pytest.raises(HeartbeatError, match=r"block index 4294967296 is outside \[0, 2\^32\)"):
        beat.encode_blocks(state, [(0, b"a" * C), (2 ** 32, b"")])
    # the signature comes first: a forged state raises whatever the blocks are
    with pytest.raises(HeartbeatError, match="Signature check or decryption failed"):
        beat.encode_blocks(_forged(state), [(1, b"a" * C), (1, b"a" * C)])
    other = sw.Swizzle(1.0, S, True, P256)                      # another owner's keys
    with pytest.raises(HeartbeatError, match="Signature check or decryption failed"):
        other.encode_blocks(state, [(0, b"a" * C)])
    assert fake.block_calls == []                               # nothing reached the library


# ------------------------------------------------------------------ patch_tag
@pytest.mark.parametrize("raw", [True, False])
def test_patch_tag_replaces_grows_and_shrinks(fake, oracle, sw, raw):
    data = _data(4 * C + 1)
    _, tag, _ = _tagged(sw, oracle, data, raw=raw)
    before = list(oracle.cxx_encode(P256, S, FK, AK, data))
    assert len(tag) == 5
    snap = bytes(tag._raw) if raw else list(tag._sigma)
    out = sw.Swizzle.patch_tag(tag, [3, 1], [7, 9])
    # raw stays raw, a list stays a list (looked at before .sigma materialises the list)
    assert (out._sigma is None and out._width == 32) if raw else (out._raw is None and out._sigma is not None)
    assert type(out) is sw.Tag
    if raw:
        assert bytes(out.raw(P256))[32:64] == (9).to_bytes(32, "big") and len(bytes(out.raw(P256))) == 5 * 32
    assert out.sigma == [before[0], 9, before[2], 7, before[4]] and len(out) == 5
    grown = sw.Swizzle.patch_tag(tag, [4, 6, 5], [1, 3, 2], nblocks=7)
    assert grown.sigma == before[:4] + [1, 2, 3]
    with pytest.raises(HeartbeatError, match="block 5 is added but not listed"):
        sw.Swizzle.patch_tag(tag, [4, 6], [1, 3], nblocks=7)
    shrunk = sw.Swizzle.patch_tag(tag, [1], [5], nblocks=2)
    assert shrunk.sigma == [before[0], 5]
    with pytest.raises(HeartbeatError, match="block index 2 is outside the tag's 2 blocks"):
        sw.Swizzle.patch_tag(tag, [2], [5], nblocks=2)
    with pytest.raises(HeartbeatError, match="2 indices for 1 values"):
        sw.Swizzle.patch_tag(tag, [0, 1], [5])
    # values as a Tag (what encode_blocks returns)
    vals = _tag(sw, [11, 12])
    out = sw.Swizzle.patch_tag(tag, [0, 2], vals)
    assert out.sigma[0] == 11 and out.sigma[2] == 12 and out.sigma[1] == before[1]
    if raw:
        with pytest.raises(HeartbeatError, match="does not fit"):
            sw.Swizzle.patch_tag(tag, [0], [1 << 256])
    assert (bytes(tag._raw) if raw else tag._sigma) == snap     # the argument is not modified
    assert tag.sigma == before
    # a patched tag serialises like any other
    assert sw.Tag.fromdict(grown.todict()).sigma == grown.sigma


# ------------------------------------------------------------------ update
@pytest.mark.parametrize("raw", [True, False])
def test_update_in_place_tail_append_truncate(fake, oracle, sw, raw):
    old = _data(5 * C + 40)
    beat, tag, state = _tagged(sw, oracle, old, raw=raw)
    snap = _snapshot(tag, state)
    old_sigma = list(oracle.cxx_encode(P256, S, FK, AK, old))

    def check(new, blocks, length):
        t2, s2 = beat.update(tag, state, blocks, length)
        assert (t2._sigma is None) == raw                       # looked at before .sigma materialises the list
        assert t2.sigma == oracle.cxx_encode(P256, S, FK, AK, new)
        assert _keys_of(beat, s2) == (FK, AK, len(new) // C + 1)          # the same two PRF keys
        assert s2.encrypted and s2.n == len(new) // C + 1 and s2._raw != state._raw      # signed again, a fresh IV
        assert sw.State.fromdict(s2.todict()).n == s2.n
        assert _snapshot(tag, state) == snap
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
    # append to a multiple of C: the empty last block is listed too, and keeps f(6) unreduced
    new = old + _data(C - 40, 9)
    assert len(new) == 6 * C
    t2, _ = check(new, _blocks_of(new, [5, 6]), len(new))
    assert t2.sigma[6] == oracle.cxx_prf_eval(FK, P256, 6)[0]
    # truncate: the new last block
    new = old[:2 * C + 17]
    t2, s2 = check(new, [(2, new[2 * C:])], len(new))
    assert len(t2) == 3
    new = b""
    check(new, [(0, b"")], 0)


def test_update_errors_and_their_order_before_any_call(fake, oracle, sw):
    old = _data(5 * C + 40)                                     # n = 6
    beat, tag, state = _tagged(sw, oracle, old)
    full = b"f" * C

    def fails(msg, blocks, length=None, st=state):
        with pytest.raises(HeartbeatError, match=msg):
            beat.update(tag, st, blocks, length)

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
    # the state's n is a u32: 2^32 blocks and more are refused, 2^32 - 1 is not (its missing blocks are)
    fails("a file of 4294967296 blocks does not fit the state's 32-bit block count", [(1, full)], (2 ** 32 - 1) * C)
    fails("a file of 4294967297 blocks does not fit", [(1, full)], 2 ** 32 * C + 5)
    fails("block index 4294967295 is outside the file's 4294967295 blocks", [(2 ** 32 - 1, b"")], (2 ** 32 - 2) * C)
    # the order: the signature, the block count, then per listed block the range and the repeat, then the
    # missing blocks, then the lengths
    fails("Signature check or decryption failed", [(9, b"")], (2 ** 32) * C, st=_forged(state))
    fails("does not fit the state's 32-bit block count", [(-1, b""), (-1, b"")], (2 ** 32) * C)
    fails("block index 9 is outside", [(1, full), (9, b""), (1, full)], 7 * C + 1)
    fails("block index 1 is listed twice", [(1, b"x"), (1, full), (9, b"")], 7 * C + 1)
    fails("block 5 must be listed", [(1, b"x")], 7 * C + 1)
    fails("block 1 has 1 bytes, not 128", [(7, b"xx"), (6, full), (5, full), (1, b"x")], 7 * C + 1)
    assert fake.block_calls == []


# ------------------------------------------------------------------ update_file
def test_update_file_equals_update_and_restores_position(fake, oracle, sw, tmp_path):
    old = _data(5 * C + 40)
    beat, tag, state = _tagged(sw, oracle, old)
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
        assert t2.sigma == oracle.cxx_encode(P256, S, FK, AK, new)
        assert _keys_of(beat, s2) == (FK, AK, 7)
        t3, _ = beat.update(tag, state, _blocks_of(new, [2, 5, 6]), len(new))
        assert t3.sigma == t2.sigma
    assert fake.block_calls == [(1, [3])] * 4
    with pytest.raises(HeartbeatError, match=r"range \(700, 1\) is outside the file's 680 bytes"):
        beat.update_file(tag, state, io.BytesIO(old), [(700, 1)])
    # a truncation without any changed range: the length rule picks the new last block
    t4, s4 = beat.update_file(tag, state, io.BytesIO(old[:C]), [])
    assert t4.sigma == oracle.cxx_encode(P256, S, FK, AK, old[:C]) and s4.n == 2


# ------------------------------------------------------------------ update_many
def test_update_many_equals_loop(fake, oracle, sw, monkeypatch):
    beat = sw.Swizzle(1.0, S, True, P256)
    items, news = [], []
    for k in range(4):
        fk, ak = bytes([k + 1]) * 32, bytes([k + 9]) * 32
        old = _data((k + 1) * C + 10 * k, k)
        sigma = oracle.cxx_encode(P256, S, fk, ak, old)
        tag, state = _tag(sw, sigma), _state(sw, beat, fk, ak, len(sigma))
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
        fk, ak = bytes([k + 1]) * 32, bytes([k + 9]) * 32
        assert t2.sigma == oracle.cxx_encode(P256, S, fk, ak, new)
        assert _keys_of(beat, s2) == (fk, ak, len(new) // C + 1)
    # below CXX_UPDATE_MANY_MIN: the loop
    monkeypatch.setattr(sw, "CXX_UPDATE_MANY_MIN", 9)
    fake.block_calls[:] = []
    tag, state = items[0][0], items[0][1]
    again = beat.update_many([(tag, state, _blocks_of(news[0], [0]), len(news[0]))] * 2)
    assert fake.block_calls == [(1, [1]), (1, [1])]
    assert again[0][0].sigma == res[0][0].sigma
    assert beat.update_many([]) == []


def test_update_many_raises_the_loops_first_error(fake, oracle, sw):
    old = _data(3 * C + 1)
    beat, tag, state = _tagged(sw, oracle, old)
    good = (tag, state, [(0, old[:C])], None)
    bad_len = (tag, state, [(1, b"short")], None)
    bad_idx = (tag, state, [(4, b"")], None)
    bad_sig = (tag, _forged(state), [(0, old[:C])], None)
    with pytest.raises(HeartbeatError, match="block 1 has 5 bytes, not 128"):
        beat.update_many([good, bad_len, bad_idx])
    with pytest.raises(HeartbeatError, match="block index 4 is outside the file's 4 blocks"):
        beat.update_many([good, bad_idx, bad_len])
    with pytest.raises(HeartbeatError, match="Signature check or decryption failed"):
        beat.update_many([good, bad_sig, bad_len])
    assert fake.block_calls == []                               # before any library call


def test_module_function_names_the_cxx_entry_point(fake, oracle, sw):
    out = sw.encode_blocks_many(P256, S, [(FK, AK, [3, 1], _data(C + 5)), (AK, FK, [], b"")])
    assert fake.block_calls == [(2, [2, 0])]
    want = [oracle.cxx_encode(P256, S, FK, AK, _data(C + 5)[k * C:(k + 1) * C], block_base=i, nblocks=1)[0]
            for k, i in enumerate([3, 1])]
    assert bytes(out[0]) == b"".join(v.to_bytes(32, "big") for v in want) and len(out[1]) == 0
    with pytest.raises(HeartbeatError):                         # the library's own refusal reaches the caller
        sw.encode_blocks_many(P256, S, [(FK, AK, [2 ** 32], b"")])
