"""heartbeat_amd.OneHash's routing of the device draw (pick_blocks_many,
generate_challenges_many(draw=...)) against a fake native library whose draw
is the rule restated in tests/onehash_draw_ref.py and whose responses are
hashlib's: which items the device takes, what stays with pick_blocks, and --
for batches that mix both and an item that fails -- the results, the
exception and random.getstate() of a loop of the single calls on the host
path.  No GPU is needed."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import fake_native
import onehash_draw_ref as R


def _ptr(d, name):
    """The address in a pointer field, whatever its ctypes type."""
    return ctypes.cast(ctypes.byref(d, getattr(type(d), name).offset), ctypes.POINTER(ctypes.c_void_p))[0]


def _part(data, block):
    """The issue's plan rule, restated."""
    fs = len(data)
    c = min(1024, fs // 10)
    if block <= fs - c:
        return data[block:block + c]
    a = block - (fs - c)
    return data[block:min(block + a, fs)] + data[:c - a]


class FakeOneHash(fake_native.FakeLib):
    """The OneHash calls on the CPU; `drawn` lists (len, num) of every file
    the device drew, `given` the num of every file whose blocks came along."""

    def __init__(self):
        super(FakeOneHash, self).__init__()
        self.drawn, self.given, self.calls = [], [], []
        self.min_jobs, self.draw_min_jobs = 256, 0

    def hb_onehash_device_min_jobs(self):
        return self.min_jobs

    def hb_onehash_draw_device_min_jobs(self):
        return self.draw_min_jobs

    def _draw(self, d):
        assert 1 <= d.key_words <= R.MAX_KEY_WORDS and (d.len >= 1 or d.num == 0)
        key = list(np.ctypeslib.as_array(ctypes.cast(_ptr(d, "key"), ctypes.POINTER(ctypes.c_uint32)),
                                         (d.key_words,)))
        g = R.Generator([int(w) for w in key])
        blocks = [g.below(d.len) for _ in range(d.num)]
        if d.num:
            ctypes.memmove(_ptr(d, "blocks_out"), np.array(blocks, dtype=np.uint64).tobytes(), 8 * d.num)
        if _ptr(d, "state_out"):
            ctypes.memmove(_ptr(d, "state_out"), np.array(g.state(), dtype=np.uint32).tobytes(), 4 * 625)
        self.drawn.append((d.len, d.num))
        return blocks

    def hb_onehash_pick_blocks_many(self, h, descs, n, flags):
        self.calls.append("pick")
        assert flags == 0
        for k in range(n):
            self._draw(descs[k])
        return 0

    def _generate(self, descs, n, seeds_out, resp_out, blocks_of):
        at = 0
        for k in range(n):
            d = descs[k]
            data = ctypes.string_at(_ptr(d, "data"), d.len) if d.len else b""
            secret = ctypes.string_at(_ptr(d, "secret"), d.secret_len) if d.secret_len else b""
            seed = ctypes.string_at(_ptr(d, "s0"), 32)
            for block in blocks_of(d):
                ctypes.memmove(_native_addr(seeds_out) + 32 * at, seed, 32)
                ctypes.memmove(_native_addr(resp_out) + 32 * at, hashlib.sha256(_part(data, block) + seed).digest(), 32)
                seed = hashlib.sha256(seed + secret).digest()
                at += 1
        return 0

    def hb_onehash_generate_drawn_many(self, h, descs, n, seeds_out, resp_out, flags):
        self.calls.append("drawn")
        return self._generate(descs, n, seeds_out, resp_out, self._draw)

    def hb_onehash_generate_many(self, h, descs, n, seeds_out, resp_out, flags):
        self.calls.append("given")

        def blocks_of(d):
            self.given.append(d.num)
            return [int(b) for b in np.ctypeslib.as_array(
                ctypes.cast(_ptr(d, "blocks"), ctypes.POINTER(ctypes.c_uint64)), (d.num,))] if d.num else []
        return self._generate(descs, n, seeds_out, resp_out, blocks_of)


def _native_addr(x):
    return x if isinstance(x, int) else fake_native._v(x)


@pytest.fixture
def fake(monkeypatch):
    from heartbeat_amd import _native
    lib = FakeOneHash()
    monkeypatch.setattr(_native, "_lib", lib)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setenv("HB_ONEHASH_DEVICE", "1")
    for name in ("HB_ONEHASH_HOST", "HB_ONEHASH_DRAW_HOST", "HB_ONEHASH_DRAW_DEVICE", "HB_DEVICES"):
        monkeypatch.delenv(name, raising=False)
    return lib


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return R.write_sized_files(tmp_path_factory.mktemp("onehash_draw_files"))


def outcome(fn):
    try:
        return fn()
    except Exception as e:
        return "!%s: %s" % (type(e).__name__, e)


def loop_pick(items):
    """The reference: a loop of pick_blocks, the results so far, what it
    raised and the generator's state."""
    from heartbeat_amd.OneHash import OneHash
    done, error = [], None
    for size, num, root in items:
        beat = OneHash.__new__(OneHash)
        beat.file_size, beat.file_object, beat._dev = size, None, None
        try:
            done.append(beat.pick_blocks(num, root))
        except Exception as e:
            error = "!%s: %s" % (type(e).__name__, e)
            break
    return done, error, random.getstate()


def many_pick(items):
    from heartbeat_amd.OneHash import OneHash
    got = outcome(lambda: OneHash.pick_blocks_many(items))
    return got, random.getstate()


# ---------------------------------------------------------------- eligibility
def test_every_seed_type_of_the_matrix_is_drawn_on_the_device(fake):
    items = [(length, num, seed) for seed in R.SEEDS for length, num in ((1000, 5), ((1 << 40) - 1, 3))]
    random.seed("elsewhere")
    want, error, state = loop_pick(items)
    random.seed("elsewhere")
    got, after = many_pick(items)
    assert error is None and got == want and after == state
    assert fake.drawn == [(length, num) for length, num, _ in items] and fake.calls == ["pick"]


def test_what_the_device_does_not_take_stays_with_pick_blocks(fake):
    """A float, an int subclass, a str that does not encode, a list, a seed
    one word above the cap, an empty file, a size of 2^64, a negative num:
    drawn by pick_blocks, with its result or its exception."""
    class MyInt(int):
        pass
    at_cap, above = b"\x01" * 4032, b"\x01" * 4033
    assert len(R.key_of(at_cap)) == R.MAX_KEY_WORDS and len(R.key_of(above)) == R.MAX_KEY_WORDS + 1
    host = [(1000, 4, 2.5), (1000, 4, MyInt(5)), (1000, 4, above), (1 << 64, 4, b"r")]
    for item in host + [(1000, 4, at_cap), (0, 0, b"r"), (1000, 0, "s")]:
        random.seed("elsewhere")
        want, error, state = loop_pick([item])
        random.seed("elsewhere")
        got, after = many_pick([item])
        assert error is None and got == want and after == state, item
    assert fake.drawn == [(1000, 4), (0, 0), (1000, 0)]
    for item, kind in (((1000, 2, "\ud800"), "UnicodeEncodeError"), ((0, 2, b"r"), "ValueError"),
                       ((1000, -1, b"r"), "HeartbeatError"), ((1000, 2, [1]), "TypeError")):
        random.seed("elsewhere")
        _, error, state = loop_pick([item])
        random.seed("elsewhere")
        got, after = many_pick([item])
        assert error.startswith("!" + kind) and got == error and after == state, item
    assert len(fake.drawn) == 3
    # None seeds from the system's entropy: nothing to compare but the range
    got, _ = many_pick([(1000, 6, None)])
    assert len(got[0]) == 6 and all(0 <= b < 1000 for b in got[0]) and len(fake.drawn) == 3


def test_host_switches_keep_every_draw_on_pick_blocks(fake, monkeypatch):
    for name in ("HB_ONEHASH_DRAW_HOST", "HB_ONEHASH_HOST"):
        monkeypatch.setenv(name, "1")
        want, _, state = loop_pick([(1000, 5, b"r")])
        got, after = many_pick([(1000, 5, b"r")])
        assert got == want and after == state and fake.calls == []
        monkeypatch.delenv(name)


# ---------------------------------------------------------------- mixed batches
DEV_A, DEV_B, DEV_C, DEV_D = (1000, 5, b"a"), (5000, 0, "s"), (1 << 33, 700, 7), (20000, 4, bytearray(b"ba"))
HOST_A, HOST_B = (1000, 3, 2.5), (5000, 2, -0.125)
FAIL_UNSEEDED, FAIL_SEEDED = (1000, -1, b"r"), (0, 2, b"r")   # raises before / after random.seed
BATCHES = [[DEV_A, HOST_A, DEV_B, DEV_C, HOST_B, DEV_D],      # a device draw decides the state
           [DEV_D, HOST_B, DEV_C, DEV_A, HOST_A],             # a host draw does
           [HOST_A, DEV_A, HOST_A]]                           # the same host draw before and after


@pytest.mark.parametrize("where", ["none", "front", "middle", "end"])
@pytest.mark.parametrize("bad", [FAIL_UNSEEDED, FAIL_SEEDED])
def test_pick_blocks_many_mixed_batches(fake, bad, where):
    for batch in BATCHES:
        items = batch if where == "none" else R.with_failure(batch, bad, where)
        random.seed("elsewhere")
        want, error, state = loop_pick(items)
        random.seed("elsewhere")
        got, after = many_pick(items)
        assert got == (want if error is None else error), (where, items)
        assert after == state, (where, items)
        assert (error is None) == (where == "none")


def _beats(paths, items, secret=b"secret"):
    from heartbeat_amd.OneHash import OneHash
    return [(OneHash(paths[size], None if root == "no secret" else secret), num, root) for size, num, root in items]


@pytest.mark.parametrize("where", ["none", "front", "middle", "end"])
@pytest.mark.parametrize("bad", R.GEN_FAILS)
def test_generate_challenges_many_mixed_batches(fake, paths, monkeypatch, bad, where):
    from heartbeat_amd.OneHash import OneHash
    for batch in R.GEN_BATCHES:
        items = batch if where == "none" else R.with_failure(batch, bad, where)
        ref = _beats(paths, items)
        monkeypatch.setenv("HB_ONEHASH_HOST", "1")
        random.seed("elsewhere")
        error = None
        for beat, num, root in ref:
            error = outcome(lambda: beat.generate_challenges(num, root))
            if error is not None:
                break
        state = random.getstate()
        monkeypatch.delenv("HB_ONEHASH_HOST")
        calls_before = len(fake.calls)
        mine = _beats(paths, items)
        random.seed("elsewhere")
        got = outcome(lambda: OneHash.generate_challenges_many(mine, draw="device"))
        assert got == error and (error is None) == (where == "none"), (where, items)
        assert random.getstate() == state, (where, items)
        for (a, _, _), (b, _, _) in zip(mine, ref):
            assert [(c.block, c.seed, c.response) for c in a.challenges] == \
                [(c.block, c.seed, c.response) for c in b.challenges], (where, items)
        if where in ("none", "end"):
            assert fake.calls[calls_before:] == ["given", "drawn"]


def test_draw_modes_and_the_internal_call(fake, paths, monkeypatch):
    """draw="host" and HB_ONEHASH_DRAW_HOST=1 keep pick_blocks; the forced GPU
    path alone and HB_ONEHASH_DRAW_DEVICE=1 draw on the device; the caller's
    draw wins; _gpu_generate is still called with (plan, chain) and
    plan[i][1] == num; an unforced call below the job floor draws nothing on
    the device and ends in the same state."""
    from heartbeat_amd.OneHash import OneHash
    items = [(1000, 5, b"a"), (20000, 9, 7)]
    want = _beats(paths, items)
    monkeypatch.setenv("HB_ONEHASH_HOST", "1")
    for beat, num, root in want:
        beat.generate_challenges(num, root)
    state = random.getstate()
    monkeypatch.delenv("HB_ONEHASH_HOST")
    seen = []
    real = OneHash._gpu_generate
    monkeypatch.setattr(OneHash, "_gpu_generate",
                        staticmethod(lambda p, chain=None: seen.append(([e[1] for e in p], chain)) or real(p, chain)))

    def run(draw=None, chain=None):
        mine = _beats(paths, items)
        del fake.calls[:]
        random.seed("elsewhere")
        OneHash.generate_challenges_many(mine, chain=chain, draw=draw)
        assert random.getstate() == state
        for (a, _, _), (b, _, _) in zip(mine, want):
            assert [(c.block, c.seed, c.response) for c in a.challenges] == \
                [(c.block, c.seed, c.response) for c in b.challenges]
        return list(fake.calls)

    assert run() == ["drawn"]                       # HB_ONEHASH_DEVICE=1 alone
    assert run(draw="host") == ["given"]
    assert run(draw="device", chain="host") == ["drawn"]
    assert seen == [([5, 9], None), ([5, 9], None), ([5, 9], "host")]
    monkeypatch.setenv("HB_ONEHASH_DRAW_HOST", "1")
    assert run() == ["given"] and run(draw="device") == ["drawn"]
    monkeypatch.delenv("HB_ONEHASH_DRAW_HOST")
    monkeypatch.delenv("HB_ONEHASH_DEVICE")
    assert run() == [] and run(draw="device") == []   # 14 jobs: the host path, whoever would have drawn
    monkeypatch.setenv("HB_ONEHASH_DRAW_DEVICE", "1")
    assert run() == []
    monkeypatch.delenv("HB_ONEHASH_DRAW_DEVICE")
    # the library's choice: a call of one file from the draw's job floor; several files only when asked
    fake.min_jobs, fake.draw_min_jobs = 4, 9
    assert run() == ["given"] and run(draw="device") == ["drawn"]
    for num, calls in ((9, ["drawn"]), (8, ["given"])):
        beat = _beats(paths, [(20000, num, 7)])[0][0]
        del fake.calls[:]
        beat.generate_challenges(num, 7)
        assert fake.calls == calls and [c.block for c in beat.challenges] == R.expected(7, 20000, num)[0]
    fake.draw_min_jobs = 0
    beat.generate_challenges(9, 7)
    assert fake.calls[-1] == "given"
    with pytest.raises(ValueError):
        OneHash.generate_challenges_many([], draw="gpu")
