"""The Merkle scheme on the GPU (heartbeat_amd.Merkle: hb_merkle_encode_many,
hb_merkle_leaves_many) against the reference's recorded outputs
(tests/golden/merkle_scheme_cases.json) and the host restatement: the seed
chain by hmac, the leaves by oracle.merkle_chunk_hash, the tree by the host
MerkleTree.  The shapes are the smallest at which each path can go wrong:
n = 1 has no tree, n = 257 crosses a workgroup of leaves and of tree lanes,
n = 3 / 5 / 9 / 65 leave empty leaf slots, tiny5 clamps the chunk, 72 files
put more than one wave on the chain kernel, and a 9 MiB host file is gathered
instead of uploaded."""
import base64
import ctypes
import hashlib
import importlib
import io

import numpy as np
import pytest

import merkle_golden as mg
from conftest import load_golden, splitmix_bytes

pytestmark = pytest.mark.gpu

G = load_golden("merkle_scheme_cases.json")
CASES = G["cases"]
HELPER = load_golden("merkle_cases.json")


@pytest.fixture(scope="module")
def M():
    from heartbeat_amd import _native
    _native.context()
    return importlib.import_module("heartbeat_amd.Merkle.Merkle")


_file = mg.file_bytes
_j = mg.plain


class Dev(object):
    """Bytes copied to the GPU, as a DeviceFile; freed on exit."""

    def __init__(self, M, data):
        from heartbeat_amd import _native
        self.ctx, self.L = _native.context(), _native.lib()
        p = ctypes.c_void_p()
        self.ctx.check(self.L.hb_device_malloc(self.ctx.h, max(1, len(data)), ctypes.byref(p)))
        self.p = p.value
        a = np.frombuffer(data, dtype=np.uint8)
        if len(a):
            self.ctx.check(self.L.hb_memcpy(self.ctx.h, self.p, a.ctypes.data, len(a), 1))
        self.file = M.DeviceFile(self.p, len(data))

    def __enter__(self):
        return self.file

    def __exit__(self, *exc):
        self.ctx.check(self.L.hb_device_free(self.ctx.h, self.p))


def _beat(M, c):
    return M.Merkle(c["check_fraction"], bytes.fromhex(c["key"]))


def _check_golden(M, c, tag, state, leaves=None):
    assert mg.tag_matches(c, tag.todict()), (c["file"], c["n"], c["chunksz"])
    assert state.root == base64.b64decode(c["state"]["root"])
    if leaves is not None:
        assert mg.leaves_match(c, [x.hex() for x in leaves])
    state.checksig(bytes.fromhex(c["key"]))            # signed by encode
    state.timestamp = G["timestamp"]
    state.sign(bytes.fromhex(c["key"]))
    assert state.todict() == c["state"]


_EXPECT = {}


def _expect(M, oracle, key, seed, n, data, chunksz, filesz=None):
    """(tree, leaves, offsets) by the host restatement; computed once per shape."""
    k = (key, seed, n, hashlib.sha256(data).digest(), chunksz, filesz)
    if k not in _EXPECT:
        fs = len(data) if filesz is None else filesz
        seeds = M.MerkleHelper.seed_chain(key, seed, n)
        t = M.MerkleTree()
        leaves = [oracle.merkle_chunk_hash(data, s, fs, chunksz) for s in seeds]
        for leaf in leaves:
            t.add_leaf(leaf)
        t.build()
        t.strip_leaves()
        _EXPECT[k] = (t, leaves, [oracle.merkle_chunk(s, fs, chunksz)[0] for s in seeds])
    return _EXPECT[k]


@pytest.mark.parametrize("chain", ["host", "device"])
@pytest.mark.parametrize("where", ["bytesio", "device"])
def test_encode_golden(M, where, chain):
    """Every golden case, from a BytesIO and from a device-resident file, with
    the seed chain forced onto the host and onto the GPU."""
    for c in CASES:
        data = _file(c["file"])
        item = lambda f: [(_beat(M, c), f, c["n"], bytes.fromhex(c["seed"]), c["chunksz"], c["filesz"])]  # noqa: E731
        if where == "bytesio":
            f = io.BytesIO(data)
            tag, state, leaves, offs = M.encode_batch(item(f), chain=chain, leaves=True)[0]
            assert f.tell() == c["file_pos_after_encode"]
        else:
            with Dev(M, data) as f:
                tag, state, leaves, offs = M.encode_batch(item(f), chain=chain, leaves=True)[0]
                assert f.tell() == c["file_pos_after_encode"]
        _check_golden(M, c, tag, state, leaves)


def test_encode_public_call_golden(M):
    """Merkle.encode itself (the runtime's own choice of chain)."""
    for c in (CASES[0], CASES[3], CASES[9], CASES[15], CASES[17], CASES[18], CASES[-1]):
        f = io.BytesIO(_file(c["file"]))
        tag, state = _beat(M, c).encode(f, c["n"], bytes.fromhex(c["seed"]), c["chunksz"], c["filesz"])
        assert f.tell() == c["file_pos_after_encode"]
        _check_golden(M, c, tag, state)
    # a random seed by default: 32 bytes, and the state is signed
    beat = M.Merkle(None, b"k" * 32)
    tag, state = beat.encode(io.BytesIO(_file("rand100k")), 3)
    assert len(state.seed) == 32 and state.n == 3 and state.index == 0
    state.checksig(beat.key)


def test_host_files_uploaded_and_gathered(M, oracle):
    """Both sides of the upload threshold max(2 n chunk, 8 MiB): a 9 MiB file
    with n = 3 and 100-byte chunks is gathered, a 1 MiB + 1 one uploaded; then
    both in one call with a golden file between them."""
    key, seed = b"K" * 32, b"S" * 32
    big = splitmix_bytes(7, 0, (9 << 20) + 5)
    small = splitmix_bytes(8, 3, (1 << 20) + 1)
    beat = M.Merkle(None, key)
    shapes = [(big, 3, 100), (small, 5, 1000)]
    for data, n, chunk in shapes:
        tag, state, leaves, offs = M.encode_batch([(beat, io.BytesIO(data), n, seed, chunk, None)], leaves=True)[0]
        tree, want_leaves, want_offs = _expect(M, oracle, key, seed, n, data, chunk)
        assert offs == want_offs and leaves == want_leaves
        assert tag.tree == tree and state.root == tree.get_root()
    c = CASES[4]
    got = M.Merkle.encode_mixed([(beat, io.BytesIO(big), 3, seed, 100),
                                 (_beat(M, c), io.BytesIO(_file(c["file"])), c["n"], bytes.fromhex(c["seed"]),
                                  c["chunksz"]),
                                 (beat, io.BytesIO(small), 5, seed, 1000),
                                 (beat, io.BytesIO(big), 2, seed, 1)])
    assert got[0][0].tree == _expect(M, oracle, key, seed, 3, big, 100)[0]
    _check_golden(M, c, *got[1])
    assert got[2][0].tree == _expect(M, oracle, key, seed, 5, small, 1000)[0]
    assert got[3][0].tree == _expect(M, oracle, key, seed, 2, big, 1)[0]
    # the prove side gathers too: one chunk of the 9 MiB file, and one proof
    # of it beside a proof of an uploaded file in one call
    tag0, state0 = got[0]
    tag2, state2 = got[2]
    chal0, chal2 = beat.gen_challenge(state0), beat.gen_challenge(state2)
    proof = beat.get_public().prove(io.BytesIO(big), chal0, tag0)
    assert proof.leaf.blob == oracle.merkle_chunk_hash(big, chal0.seed, len(big), 100)
    assert beat.verify(proof, chal0, state0)
    both = M.Merkle.prove_many([(io.BytesIO(small), chal2, tag2), (io.BytesIO(big), chal0, tag0)])
    assert both[1] == proof and beat.verify(both[0], chal2, state2)


def _mixed_items(M):
    """72 files of many owners: every golden case, then slices of rand100k
    under keys of 0, 16, 32 and 70 bytes with mixed n, chunk sizes and lengths."""
    base = _file("rand100k")
    items = [(_beat(M, c), _file(c["file"]), c["n"], bytes.fromhex(c["seed"]), c["chunksz"])
             for c in CASES if c["filesz"] is None]
    ns = (1, 2, 3, 5, 8, 9, 17, 64, 65, 130)
    chunks = (8192, 100, 1, 4097, 0, None)
    k = 0
    while len(items) < 72:
        key = hashlib.sha256(b"owner%d" % k).digest() * 3
        key = key[:(0, 16, 32, 70)[k % 4]]
        length = (0, 5, 63, 64, 65, 1000, 8191, 8192, 8193, 50000, 100003)[k % 11]
        frac = 0.05 if chunks[k % 6] is None else None
        items.append((M.Merkle(frac, key), base[k:k + length], ns[k % 10],
                      hashlib.sha256(b"seed%d" % k).digest()[:(32, 5, 0)[k % 3]], chunks[k % 6]))
        k += 1
    return items


def test_encode_mixed_is_the_loop_and_the_goldens(M, oracle):
    items = _mixed_items(M)
    assert len(items) >= 70
    got = M.Merkle.encode_mixed([(m, io.BytesIO(d), n, s, c) for m, d, n, s, c in items])
    # the loop of single encodes, chains on the host there and on the GPU in the batch
    for (m, d, n, s, c), (tag, state) in zip(items, got):
        t1, s1 = m.encode(io.BytesIO(d), n, s, c)
        s1.timestamp = state.timestamp
        s1.sign(m.key)
        assert t1 == tag and s1 == state and (tag.chunksz, tag.filesz) == (t1.chunksz, len(d))
    golden = [c for c in CASES if c["filesz"] is None]
    for c, (tag, state) in zip(golden, got):
        _check_golden(M, c, tag, state)
    # and the host restatement for the files that are not golden
    for (m, d, n, s, c), (tag, state) in list(zip(items, got))[len(golden)::7]:
        tree = _expect(M, oracle, m.key, s, n, d, tag.chunksz)[0]
        assert tag.tree == tree
    # device-resident, the same batch
    devs = [Dev(M, d) for _, d, _, _, _ in items]
    try:
        again = M.Merkle.encode_mixed([(m, dv.file, n, s, c) for (m, d, n, s, c), dv in zip(items, devs)])
    finally:
        for dv in devs:
            dv.__exit__()
    assert [t.todict() for t, _ in again] == [t.todict() for t, _ in got]
    assert [st.root for _, st in again] == [st.root for _, st in got]


def test_encode_many_one_owner(M):
    beat = M.Merkle(None, b"owner-key" * 3)
    base = _file("rand100k")
    datas = [base[7 * k:7 * k + 3000 + 11 * k] for k in range(70)]
    seeds = [hashlib.sha256(b"s%d" % k).digest() for k in range(70)]
    files = [io.BytesIO(d) for d in datas]
    got = beat.encode_many(files, 4, seeds, 100)
    assert len(got) == 70
    for k in (0, 1, 33, 69):
        f = io.BytesIO(datas[k])
        tag, state = beat.encode(f, 4, seeds[k], 100)
        assert tag == got[k][0] and state.root == got[k][1].root and f.tell() == files[k].tell()
    assert beat.encode_many([]) == [] and M.Merkle.encode_mixed([]) == []
    with pytest.raises(M.HeartbeatError):
        beat.encode_many(files, 4, seeds[:3], 100)
    # random seeds by default, one per file
    rnd = beat.encode_many([io.BytesIO(datas[0]), io.BytesIO(datas[0])], 2)
    assert rnd[0][1].seed != rnd[1][1].seed


def test_default_shape(M, oracle):
    """A 1 MiB file, n = 256, chunks of 8192 bytes."""
    data = splitmix_bytes(11, 0, 1 << 20)
    key, seed = b"k" * 32, b"s" * 32
    f = io.BytesIO(data)
    tag, state = M.Merkle(None, key).encode(f, seed=seed)
    tree, leaves, offs = _expect(M, oracle, key, seed, 256, data, 8192)
    assert tag.tree == tree and state.root == tree.get_root() and state.n == 256
    assert (tag.chunksz, tag.filesz) == (8192, 1 << 20) and f.tell() == offs[-1] + 8192


def test_prove_golden(M):
    """Every golden proof in one prove_many call, host files and device files;
    single proves for a few; verify is true for all of them.  The tags are
    this build's (a large case's is recorded as a digest) once they match."""
    per_case, items = [], []
    for c in CASES:
        beat = _beat(M, c)
        tag, state = beat.encode(io.BytesIO(_file(c["file"])), c["n"], bytes.fromhex(c["seed"]), c["chunksz"],
                                 c["filesz"])
        assert mg.tag_matches(c, tag.todict())
        state = M.State.fromdict(c["state"])
        chals = [beat.gen_challenge(state) for _ in range(c["n"])]
        assert mg.challenges_match(c, [ch.todict() for ch in chals])
        per_case.append((c, beat, state, chals, len(items)))
        items += [(c, ch, tag) for ch in chals]
    got = M.Merkle.prove_many([(io.BytesIO(_file(c["file"])), ch, tag) for c, ch, tag in items])
    for c, beat, state, chals, at in per_case:
        mine = got[at:at + c["n"]]
        assert mg.proofs_match(c, [p.todict() for p in mine]), (c["file"], c["n"])
        assert all(beat.verify(p, ch, state) for ch, p in zip(chals, mine))
    devs = {name: Dev(M, _file(name)) for name in G["files"]}
    try:
        sub = list(zip(items, got))[::5]
        again = M.Merkle.prove_many([(devs[c["file"]].file, ch, tag) for (c, ch, tag), _ in sub])
        assert again == [w for _, w in sub]
        for (c, ch, tag), w in sub[::40]:
            f = io.BytesIO(_file(c["file"]))
            assert _beat(M, c).get_public().prove(f, ch, tag) == w
            chunk = min(tag.chunksz, tag.filesz)
            assert chunk <= f.tell() <= tag.filesz                  # left after the chunk
            assert M.Merkle().prove(devs[c["file"]].file, ch, tag) == w
    finally:
        for dv in devs.values():
            dv.__exit__()


def test_prove_seed_lengths_in_one_call(M):
    """Seeds of 16, 24 and 32 bytes interleaved in one call (a launch per
    length, results back in the caller's order), against the reference's
    recorded leaves."""
    data = _file("rand100k")
    tag = M.Tag(M.MerkleTree._from_raw(bytes(64), 0, 1), 8192, None)
    by_len = {}
    for c in HELPER["cases"]:
        if c["file"] == "rand100k" and c["chunksz"] == 8192:
            by_len.setdefault(len(c["seeds"][0]) // 2, c)
    assert set(by_len) == {16, 24, 32}
    pairs = [(bytes.fromhex(s), leaf) for k in range(12) for c in by_len.values()
             for s, leaf in [(c["seeds"][k], c["leaves"][k])]]
    got = M.Merkle.prove_many([(io.BytesIO(data), M.Challenge(s, 0), tag) for s, _ in pairs])
    assert [p.leaf.blob.hex() for p in got] == [leaf for _, leaf in pairs]
    with pytest.raises(M.HeartbeatError, match="16, 24, or 32"):
        M.Merkle().prove(io.BytesIO(data), M.Challenge(b"short", 0), tag)


def test_full_flow(M):
    data = _file("rand100k")
    beat = M.Merkle(None, b"flow-key" * 4)
    tag, state = beat.encode(io.BytesIO(data), 9, chunksz=500)
    tag = M.Tag.fromdict(_j(tag.todict()))
    server = M.Merkle.fromdict(beat.get_public().todict())
    for i in range(9):
        state = M.State.fromdict(_j(state.todict()))
        chal = beat.gen_challenge(state)
        assert chal.index == i
        proof = M.Proof.fromdict(_j(server.prove(io.BytesIO(data), M.Challenge.fromdict(chal.todict()), tag).todict()))
        assert beat.verify(proof, chal, state)
        # another file of the same length does not pass
        assert not beat.verify(server.prove(io.BytesIO(data[::-1]), chal, tag), chal, state)
    with pytest.raises(M.HeartbeatError, match="Out of challenges."):
        beat.gen_challenge(state)


def test_errors_before_any_launch(M):
    from heartbeat_amd import _native
    beat = M.Merkle(None, b"k" * 32)
    data = _file("test.txt")
    with pytest.raises(M.HeartbeatError, match="chunk past the end of the data"):
        beat.encode(io.BytesIO(data), 4, b"s" * 32, 100, len(data) + 1)
    for n in (0, 65537):
        with pytest.raises(M.HeartbeatError, match="n must be in 1..65536"):
            beat.encode(io.BytesIO(data), n)
    with pytest.raises(M.HeartbeatError, match="chunk past the end of the data"):
        tag = M.Tag(M.MerkleTree._from_raw(bytes(64), 0, 1), 100, len(data) + 1)
        beat.prove(io.BytesIO(data), M.Challenge(b"c" * 32, 0), tag)
    # the C ABI's own checks, made before the first launch
    ctx, L = _native.context(), _native.lib()
    arr = np.frombuffer(data, dtype=np.uint8)
    nodes = np.zeros(2 * 65536 * 2 * 32, dtype=np.uint8)
    key = seed = b"x" * 32

    def call(n, filesz, length, flags=0, nodes_ptr=None):
        d = (_native.MerkleEncodeDesc * 1)()
        d[0].key, d[0].key_len, d[0].seed, d[0].seed_len = key, 32, seed, 32
        d[0].n, d[0].filesz, d[0].chunksz = n, filesz, 100
        d[0].data, d[0].len = arr.ctypes.data, length
        d[0].nodes_out = nodes.ctypes.data if nodes_ptr is None else nodes_ptr
        with ctx.lock:
            rc = L.hb_merkle_encode_many(ctx.h, d, 1, flags)
        return rc, L.hb_last_error(ctx.h).decode()

    assert call(0, len(data), len(data))[0] == -1 and "1..65536" in call(0, len(data), len(data))[1]
    assert call(65537, len(data), len(data))[0] == -1
    assert call(4, len(data) + 1, len(data)) == (-1, "chunk past the end of the data")
    assert call(4, len(data), len(data), flags=64 | 128)[0] == -1
    assert call(4, len(data), len(data), flags=2)[0] == -1
    assert call(4, len(data), len(data), nodes_ptr=0) == (-1, "NULL buffer")
    assert call(4, len(data), len(data))[0] == 0                   # and the same descriptor, valid
    with ctx.lock:
        assert L.hb_merkle_encode_many(ctx.h, None, 0, 0) == 0     # the empty batch
        assert L.hb_merkle_leaves_many(ctx.h, None, 0, 0) == 0
