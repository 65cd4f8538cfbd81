"""The OneHash device draw on the GPU (hb_onehash_draw_kernel through
hb_onehash_pick_blocks_many, hb_onehash_generate_drawn_many and
heartbeat_amd.OneHash) against Python's own ``random`` at test time:
random.seed(root), randint(0, len - 1) num times, random.getstate().  The
matrix of tests/onehash_draw_ref.py in one call -- ranges of one value, round
2^32 and up to 2^64 - 1, keys of 1 to 41 words, counts on both sides of one
and two regenerations, the draw that ends exactly on a regeneration -- and
generate_challenges_many with the positions drawn on the device against the
same call with pick_blocks, on the golden files."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import onehash_draw_ref as R
import onehash_golden as og
from conftest import load_golden, splitmix_bytes

pytestmark = pytest.mark.gpu

G = load_golden("onehash_cases.json")
NAMES = list(G["files"])


@pytest.fixture(autouse=True)
def gpu_path(monkeypatch):
    monkeypatch.setenv("HB_ONEHASH_DEVICE", "1")
    for name in ("HB_ONEHASH_HOST", "HB_ONEHASH_DRAW_HOST", "HB_ONEHASH_DRAW_DEVICE"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def O():
    from heartbeat_amd import _native
    _native.context()
    import heartbeat_amd.OneHash
    return heartbeat_amd.OneHash


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return og.write_files(tmp_path_factory.mktemp("onehash_files"), NAMES)


@pytest.fixture(scope="module")
def sized(tmp_path_factory):
    return R.write_sized_files(tmp_path_factory.mktemp("onehash_draw_files"))


@pytest.fixture(scope="module")
def devs():
    """The golden files in GPU memory: {name: (pointer, length)}."""
    from heartbeat_amd import _native
    ctx, L = _native.context(), _native.lib()
    made = {}
    for n in NAMES:
        data = np.frombuffer(og.file_bytes(n), dtype=np.uint8)
        p = ctypes.c_void_p()
        ctx.check(L.hb_device_malloc(ctx.h, max(1, len(data)), ctypes.byref(p)))
        if len(data):
            ctx.check(L.hb_memcpy(ctx.h, p.value, data.ctypes.data, len(data), 1))
        made[n] = (p.value, len(data))
    yield made
    for p, _ in made.values():
        ctx.check(L.hb_device_free(ctx.h, p))


def raw_draw(cases, poison=0):
    """hb_onehash_pick_blocks_many over (len, num, seed) cases with every
    state asked for: (rc, blocks per file, states per file)."""
    from heartbeat_amd import _native
    ctx, L = _native.context(), _native.lib()
    total = sum(num for _, num, _ in cases)
    blocks = np.full(max(1, total), poison, dtype=np.uint64)
    states = np.full((len(cases), 625), poison, dtype=np.uint32)
    descs = (_native.OneHashDrawDesc * len(cases))()
    keys, at = [], 0
    for k, (d, (length, num, seed)) in enumerate(zip(descs, cases)):
        key = np.array(R.key_of(seed), dtype=np.uint32)
        keys.append(key)
        d.len, d.key, d.key_words, d.num = length, key.ctypes.data, len(key), num
        d.blocks_out = blocks.ctypes.data + 8 * at if num else None
        d.state_out = states[k].ctypes.data
        at += num
    rc = L.hb_onehash_pick_blocks_many(ctx.h, descs, len(cases), 0)
    out, at = [], 0
    for _, num, _ in cases:
        out.append(blocks[at:at + num].tolist())
        at += num
    return rc, out, states.tolist()


@pytest.fixture(scope="module")
def matrix():
    """The matrix and the lazy-twist case, with what Python's generator gives."""
    cases = R.matrix() + [R.LAZY]
    return cases, [R.expected(seed, length, num) for length, num, seed in cases]


def test_matrix_in_one_call(O, matrix):
    """551 files, a workgroup each: blocks through the Python call, which
    leaves the generator in the last file's state -- the draw that consumed
    exactly 624 words: index 624 on the first array."""
    cases, want = matrix
    assert want[-1][1][624] == 624   # the precondition, from random.getstate() itself
    random.seed("elsewhere")
    got = O.OneHash.pick_blocks_many(cases)
    assert random.getstate() == (3, tuple(want[-1][1]), None)
    for c, g, (blocks, _) in zip(cases, got, want):
        assert g == blocks, c


def test_matrix_states_through_the_abi(O, matrix):
    """The same call on the C ABI with every file's final state."""
    cases, want = matrix
    rc, blocks, states = raw_draw(cases)
    assert rc == 0
    for c, b, s, (wb, ws) in zip(cases, blocks, states, want):
        assert b == wb and s == ws, c


def test_130_files(O):
    cases = [((1, 1000, 1 << 33)[k % 3], (0, 1, 3, 700)[k % 4], b"file-%d" % k) for k in range(130)]
    rc, blocks, states = raw_draw(cases)
    assert rc == 0
    for (length, num, seed), b, s in zip(cases, blocks, states):
        assert (b, s) == R.expected(seed, length, num), (length, num, seed)
    assert O.OneHash.pick_blocks_many(cases) == blocks
    assert list(random.getstate()[1]) == states[-1]


def _beat(O, where, paths, devs, name, secret):
    if where == "device":
        return O.OneHash.from_device(devs[name][0], devs[name][1], secret)
    return O.OneHash(paths[name], secret)


def _both_draws(O, make_items, chain):
    """generate_challenges_many with draw="host" and draw="device": the
    challenges and the generator's state of both."""
    out = []
    for draw in ("host", "device"):
        items = make_items()
        random.seed("elsewhere")
        O.OneHash.generate_challenges_many(items, chain=chain, draw=draw)
        out.append(([[(c.block, c.seed, c.response) for c in b.challenges] for b, _, _ in items], random.getstate()))
    return out


@pytest.mark.parametrize("chain", ["host", "device"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_generate_drawn_equals_generate_on_the_golden_files(O, where, chain, paths, devs, monkeypatch):
    """72 files x 3 in one call and one file x 300, from disk and
    device-resident, either chain: identical blocks, seeds, responses and
    generator state, and the recorded results."""
    cases = [c for c in G["generate"] if c["num"] == 3 and "error" not in c]
    cases = [cases[k % len(cases)] for k in range(72)]
    big = next(c for c in G["generate"] if c["num"] == 300 and c["file"] == "det100003" and "error" not in c)
    from heartbeat_amd import _native
    L, calls = _native.lib(), []
    real = L.hb_onehash_generate_drawn_many
    monkeypatch.setattr(L, "hb_onehash_generate_drawn_many", lambda *a: calls.append(a[2]) or real(*a))
    for group in (cases, [big]):
        def make():
            return [(_beat(O, where, paths, devs, c["file"], bytes.fromhex(c["secret"])), c["num"],
                     og.root_seed_of(c["root_seed"])) for c in group]
        (host, host_state), (dev, dev_state) = _both_draws(O, make, chain)
        assert dev == host and dev_state == host_state
        for c, got in zip(group, dev):
            assert og.matches(c["blocks"], [b for b, _, _ in got])
            assert og.matches(c["responses"], [r.hex() for _, _, r in got])
    # the device drew: one call a group, for the files whose root seed is no float
    assert calls == [sum(c["root_seed"]["t"] != "float" for c in cases), 1]


def _plan(fs, block):
    c = min(1024, fs // 10)
    if block <= fs - c:
        return [(block, block + c)]
    a = block - (fs - c)
    return [(block, min(block + a, fs)), (0, c - a)]


def _expect(data, block, seed):
    return hashlib.sha256(b"".join(data[lo:hi] for lo, hi in _plan(len(data), block)) + seed).digest()


def test_gathered_host_file(O, tmp_path):
    """A 9 MiB host file with 3 challenges lies above the upload threshold
    (8 MiB): the host gathers its segments, so the positions come down before
    the gather."""
    data = splitmix_bytes(11, 0, (9 << 20) + 7)
    p = tmp_path / "big.bin"
    p.write_bytes(data)
    (host, host_state), (dev, dev_state) = _both_draws(O, lambda: [(O.OneHash(str(p), b"secret"), 3, b"root")], None)
    want_blocks, _ = R.expected(b"root", len(data), 3)
    assert [b for b, _, _ in dev[0]] == want_blocks
    assert [r for _, _, r in dev[0]] == [_expect(data, b, s) for b, s, _ in dev[0]]
    assert dev == host and dev_state == host_state


@pytest.mark.parametrize("where", ["none", "front", "middle", "end"])
def test_mixed_batches_on_the_library(O, sized, monkeypatch, where):
    """Device-drawn items, host-drawn items and one the reference fails on:
    results, exception and generator state of a loop on the host path."""
    for bad in R.GEN_FAILS:
        for batch in R.GEN_BATCHES:
            items = batch if where == "none" else R.with_failure(batch, bad, where)

            def beats():
                return [(O.OneHash(sized[size], None if root == "no secret" else b"secret"), num, root)
                        for size, num, root in items]
            ref, error = beats(), None
            monkeypatch.setenv("HB_ONEHASH_HOST", "1")
            random.seed("elsewhere")
            for beat, num, root in ref:
                try:
                    beat.generate_challenges(num, root)
                except Exception as e:
                    error = e
                    break
            state = random.getstate()
            monkeypatch.delenv("HB_ONEHASH_HOST")
            mine = beats()
            random.seed("elsewhere")
            if error is None:
                O.OneHash.generate_challenges_many(mine, draw="device")
            else:
                with pytest.raises(type(error)) as ex:
                    O.OneHash.generate_challenges_many(mine, draw="device")
                assert str(ex.value) == str(error)
            assert random.getstate() == state, (where, items)
            for (a, _, _), (b, _, _) in zip(mine, ref):
                assert [(c.block, c.seed, c.response) for c in a.challenges] == \
                    [(c.block, c.seed, c.response) for c in b.challenges], (where, items)


def test_the_abi_refuses_bad_descriptors_and_writes_nothing(O):
    """Each refusal names the file's index, leaves every output as it was,
    and the context serves a good call afterwards."""
    from heartbeat_amd import _native
    ctx, L = _native.context(), _native.lib()
    good = [(1000, 3, b"a"), (1000, 2, b"b")]
    POISON = 0x5a5a5a5a

    def draw(text, code, len1=1000, words=None, null=None, flags=0):
        cases = [good[0], (len1,) + good[1][1:]]
        blocks = np.full(8, POISON, dtype=np.uint64)
        states = np.full((2, 625), POISON, dtype=np.uint32)
        descs = (_native.OneHashDrawDesc * 2)()
        keys = [np.array(R.key_of(seed), dtype=np.uint32) for _, _, seed in cases]
        for k, (d, (length, num, _)) in enumerate(zip(descs, cases)):
            d.len, d.key, d.key_words, d.num = length, keys[k].ctypes.data, len(keys[k]), num
            d.blocks_out, d.state_out = blocks[3 * k:].ctypes.data, states[k].ctypes.data
        if words is not None:
            descs[1].key_words = words
        if null is not None:
            setattr(descs[1], null, None)
        rc = L.hb_onehash_pick_blocks_many(ctx.h, descs, 2, flags)
        assert rc == code, (text, rc)
        msg = L.hb_last_error(ctx.h).decode()
        assert text in msg and (flags or "file 1: " in msg), msg
        assert (blocks == POISON).all() and (states == POISON).all(), text

    draw("empty range", -1, len1=0)
    draw("empty key", -1, words=0)
    draw("NULL", -1, null="key")
    draw("NULL", -1, null="blocks_out")
    draw("more than 1024 words", -4, words=1025)
    draw("unsupported flags", -1, flags=1)
    rc, blocks, states = raw_draw(good)
    assert rc == 0 and [(b, s) for b, s in zip(blocks, states)] == [R.expected(s, n, k) for n, k, s in good]
    assert L.hb_onehash_pick_blocks_many(ctx.h, None, 0, 0) == 0

    data = np.frombuffer(og.file_bytes("det1000"), dtype=np.uint8)
    s0 = hashlib.sha256(b"r").digest()

    def gen(text, code, len1=1000, words=None, null=None, flags=0):
        seeds, resp = np.full(160, 0x5a, dtype=np.uint8), np.full(160, 0x5a, dtype=np.uint8)
        blocks = np.full(8, POISON, dtype=np.uint64)
        states = np.full((2, 625), POISON, dtype=np.uint32)
        key = np.array(R.key_of(b"r"), dtype=np.uint32)
        d = (_native.OneHashDrawnDesc * 2)()
        for k in range(2):
            d[k].data, d[k].len, d[k].s0, d[k].secret, d[k].secret_len = data.ctypes.data, 1000, s0, b"sec", 3
            d[k].num, d[k].key, d[k].key_words = 2, key.ctypes.data, len(key)
            d[k].blocks_out, d[k].state_out = blocks[2 * k:].ctypes.data, states[k].ctypes.data
        d[1].len = len1
        if words is not None:
            d[1].key_words = words
        if null is not None:
            setattr(d[1], null, None)
        rc = L.hb_onehash_generate_drawn_many(ctx.h, d, 2, seeds.ctypes.data, resp.ctypes.data, flags)
        assert rc == code, (text, rc)
        if code:
            msg = L.hb_last_error(ctx.h).decode()
            assert text in msg and (flags or "file 1: " in msg), msg
            assert (blocks == POISON).all() and (states == POISON).all() and (seeds == 0x5a).all() \
                and (resp == 0x5a).all(), text
        return blocks.tolist(), states.tolist(), seeds.tobytes(), resp.tobytes()

    gen("empty range", -1, len1=0)
    gen("empty key", -1, words=0)
    gen("more than 1024 words", -4, words=1025)
    for field in ("key", "blocks_out", "s0", "secret"):
        gen("NULL", -1, null=field)
    gen("unsupported flags", -1, flags=64 | 128)
    gen("unsupported flags", -1, flags=2)
    blocks, states, seeds, resp = gen("", 0)
    want_blocks, want_state = R.expected(b"r", 1000, 2)
    s1 = hashlib.sha256(s0 + b"sec").digest()
    assert blocks[:4] == want_blocks * 2 and states == [want_state] * 2
    assert seeds[:128] == (s0 + s1) * 2
    assert resp[:64] == _expect(data.tobytes(), want_blocks[0], s0) + _expect(data.tobytes(), want_blocks[1], s1)
