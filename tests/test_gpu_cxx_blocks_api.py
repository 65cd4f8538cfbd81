"""The listed-block update of the cxx Swizzle through the public API on the GPU
(heartbeat.Heartbeat: update, update_file, update_many, encode_blocks +
patch_tag): a 300-block file at the cxx defaults (1024-bit prime, 10 sectors);
an edit of 3 scattered blocks, an append that ends on a multiple of the block
size (its empty last block keeps F unreduced) and a truncation.  After each,
through update and through update_file:

* the new tag == hb_encode(HB_PRF_CXX) of the new file under the state's keys,
* verify(prove(new file, chal, new tag), chal, new state) is True,
* a proof made from the OLD file under the new state is False,
* the arguments are as they were.

update_many of 8 items == a loop of update.

Reference: cxx/shacham_waters_private.cxx:638-702 (encode) over the new bytes
under the same keys -- the library's own hb_encode(HB_PRF_CXX), which
tests/test_gpu_cxx.py holds against the oracle's restatement."""
import io

import numpy as np
import pytest

from test_gpu_cxx import P1024
from test_gpu_cxx_blocks import whole_file

pytestmark = pytest.mark.gpu

NB = 300


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def tagged(nat):
    """The beat and the tagged file: encoded once, shared, never modified."""
    import heartbeat
    beat = heartbeat.Heartbeat(1.0, 10, True, P1024)
    C = beat.sectors * beat.sectorsize
    old = np.random.default_rng(NB).integers(0, 256, (NB - 1) * C + C // 3, dtype=np.uint8).tobytes()
    tag, state = beat.encode(io.BytesIO(old))
    assert len(tag) == NB and state.n == NB
    return beat, C, old, tag, state


def _edit(op, old, C):
    """(new bytes, changed ranges of the new file, blocks update() needs)."""
    if op == "scattered":
        new = bytearray(old)
        spots = [5, (NB // 2) * C + 1, (NB - 2) * C + C - 1]
        for s in spots:
            new[s] ^= 0x5a
        return bytes(new), [(s, 1) for s in spots], [s // C for s in spots]
    if op == "append":                                          # up to a multiple of C: blocks n - 1, n and the empty n + 1
        extra = np.random.default_rng(7).integers(0, 256, C - len(old) % C + C, dtype=np.uint8).tobytes()
        new = old + extra
        assert len(new) % C == 0
        return new, [(len(old), len(extra))], list(range(NB - 1, len(new) // C + 1))
    new = old[:len(old) // 2]                                   # truncate
    return new, [], [len(new) // C]


def _keys(beat, state):
    s = state._copy()
    assert s._check_sig_and_decrypt(beat.k_enc, beat.k_mac)
    return bytes(s.f_key), bytes(s.alpha_key), s.n


@pytest.mark.parametrize("op", ["scattered", "append", "truncate"])
def test_update_after_each_operation(nat, tagged, op):
    import heartbeat
    beat, C, old, tag, state = tagged
    old_raw, old_state = bytes(tag.raw(P1024)), state._serialize()
    new, changed, idx = _edit(op, old, C)
    blocks = [(i, new[i * C:(i + 1) * C]) for i in idx]
    length = None if op == "scattered" else len(new)
    fk, ak, n = _keys(beat, state)
    want = whole_file(nat, P1024, beat.sectors, fk, ak, new)
    n_new = len(new) // C + 1

    f = io.BytesIO(new)
    f.seek(3)
    results = [beat.update(tag, state, reversed(blocks), length), beat.update_file(tag, state, f, changed)]
    assert f.tell() == 3
    for tag2, state2 in results:
        assert bytes(tag2.raw(P1024)) == want and len(tag2) == n_new
        assert _keys(beat, state2) == (fk, ak, n_new)           # the same two PRF keys, the new block count
        assert state2.encrypted and state2._serialize() != old_state
        chal = beat.gen_challenge(state2)
        assert chal.chunks == n_new                             # check_fraction 1.0: every block
        pub = beat.get_public()
        assert beat.verify(pub.prove(io.BytesIO(new), chal, tag2), chal, state2) is True
        assert beat.verify(pub.prove(io.BytesIO(old), chal, tag2), chal, state2) is False
    assert bytes(tag.raw(P1024)) == old_raw and state._serialize() == old_state      # the arguments are as they were
    # the owner's patch applied by the server
    idx4, patch = beat.encode_blocks(state, blocks)
    assert idx4 == idx
    assert bytes(heartbeat.Heartbeat.patch_tag(tag, idx4, patch, n_new).raw(P1024)) == want
    if op == "append":                                          # the empty last block's tag is F unreduced: no MAC touched it
        assert patch.sigma[-1] == int.from_bytes(want[-128:], "big")


def test_update_many_equals_loop(nat, tagged):
    from heartbeat_amd.exc import HeartbeatError
    beat, C, old, tag, state = tagged
    items = []
    for op in ["scattered", "append", "truncate", "scattered", "truncate", "append", "scattered", "append"]:
        new, _, idx = _edit(op, old, C)
        items.append((tag, state, [(i, new[i * C:(i + 1) * C]) for i in idx], len(new)))
    res = beat.update_many(items)
    loop = [beat.update(*item) for item in items]
    assert len(res) == 8
    for (t, s), (t1, s1) in zip(res, loop):
        assert bytes(t.raw(P1024)) == bytes(t1.raw(P1024))
        assert _keys(beat, s) == _keys(beat, s1)
    with pytest.raises(HeartbeatError, match="block index 500 is outside"):
        beat.update_many(items[:2] + [(tag, state, [(500, b"")], None)] + items[2:])
