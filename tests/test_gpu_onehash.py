"""The OneHash scheme on the GPU (heartbeat_amd.OneHash: hb_onehash_meet_many,
hb_onehash_generate_many), GPU path forced, against the reference's recorded
outputs (tests/golden/onehash_cases.json).  The shapes are the smallest at
which each path can go wrong: files of 0 to 11 bytes (no chunk, a chunk of one
byte), 10239 / 10240 / 10241 bytes (the chunk reaches 1 KiB), blocks on both
sides of the wrap and of the reference's short read, seeds that put the
padding in every corner; all files in one call (mixed chunk lengths in one
wave, more than 256 jobs); 72 files (more than one wave of chains, secrets on
both sides of the device chain's 87 bytes); a 9 MiB host file that is gathered
instead of uploaded."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import onehash_golden as og
from conftest import load_golden, splitmix_bytes

pytestmark = pytest.mark.gpu

G = load_golden("onehash_cases.json")
NAMES = list(G["files"])


@pytest.fixture(autouse=True)
def gpu_path(monkeypatch):
    monkeypatch.setenv("HB_ONEHASH_DEVICE", "1")
    monkeypatch.delenv("HB_ONEHASH_HOST", raising=False)


@pytest.fixture(scope="module")
def O():
    from heartbeat_amd import _native
    _native.context()
    import heartbeat_amd.OneHash
    return heartbeat_amd.OneHash


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return og.write_files(tmp_path_factory.mktemp("onehash_files"), NAMES)


class Dev(object):
    """Bytes copied to the GPU; freed on exit."""

    def __init__(self, data):
        from heartbeat_amd import _native
        self.ctx, self.L = _native.context(), _native.lib()
        p = ctypes.c_void_p()
        self.ctx.check(self.L.hb_device_malloc(self.ctx.h, max(1, len(data)), ctypes.byref(p)))
        self.p, self.len = p.value, len(data)
        a = np.frombuffer(data, dtype=np.uint8)
        if len(a):
            self.ctx.check(self.L.hb_memcpy(self.ctx.h, self.p, a.ctypes.data, len(a), 1))

    def free(self):
        self.ctx.check(self.L.hb_device_free(self.ctx.h, self.p))


@pytest.fixture(scope="module")
def devs():
    made = {n: Dev(og.file_bytes(n)) for n in NAMES}
    yield made
    for d in made.values():
        d.free()


def _beat(O, where, paths, devs, name, secret=None):
    if where == "device":
        return O.OneHash.from_device(devs[name].p, devs[name].len, secret)
    return O.OneHash(paths[name], secret)


def _meet_cases(name):
    """(block, seed, response) of every golden case of a file that returns."""
    return [(c["block"], og.seed_of(int(sl)), r) for c in G["meet"] if c["file"] == name
            for sl, r in c["answers"].items() if not r.startswith("!")]


def _plan(fs, block):
    """The issue's rule, restated: the file part of an in-range block."""
    c = min(1024, fs // 10)
    if block <= fs - c:
        return [(block, block + c)]
    a = block - (fs - c)
    return [(block, min(block + a, fs)), (0, c - a)]


def _expect(data, block, seed):
    return hashlib.sha256(b"".join(data[lo:hi] for lo, hi in _plan(len(data), block)) + seed).digest()


@pytest.mark.parametrize("where", ["host", "device"])
def test_meet_challenges_golden(O, where, paths, devs):
    """Every golden response of every file, a call per file: the GPU's jobs and,
    in the same call, what the host path keeps (blocks file_size and
    file_size + 1, seeds of 65 and 100 bytes)."""
    gpu_jobs = 0
    for name in NAMES:
        beat = _beat(O, where, paths, devs, name)
        cases = _meet_cases(name)
        chals = [O.Challenge(b, s) for b, s, _ in cases]
        gpu_jobs += sum(beat._gpu_takes(c) for c in chals)
        got = beat.meet_challenges(chals)
        assert [r.hex() for r in got] == [r for _, _, r in cases], name
        if cases and beat._gpu_takes(chals[0]):
            assert beat.meet_challenge(chals[0]).hex() == cases[0][2]
    assert gpu_jobs > 900


def test_meet_many_all_files_in_one_call(O, paths):
    """All golden files in one launch, their jobs interleaved: lanes of one
    wave belong to files of different chunk lengths, several workgroups."""
    beats = {n: O.OneHash(paths[n]) for n in NAMES}
    jobs = [(n, b, s, r) for n in NAMES for b, s, r in _meet_cases(n) if 0 <= b < beats[n].file_size and len(s) <= 64]
    random.Random(5).shuffle(jobs)
    assert len(jobs) > 256
    got = O.OneHash.meet_many([(beats[n], O.Challenge(b, s)) for n, b, s, _ in jobs])
    assert [r.hex() for r in got] == [r for _, _, _, r in jobs]


@pytest.mark.parametrize("chain", ["host", "device"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_generate_challenges_golden(O, where, chain, paths, devs):
    """Every golden generate_challenges case: blocks, seeds, responses, the
    generator's next draw, and the reference's exceptions."""
    for c in G["generate"]:
        secret = None if c["secret"] is None else bytes.fromhex(c["secret"])
        beat = _beat(O, where, paths, devs, c["file"], secret)
        key = (c["file"], c["num"], c["root_seed"]["t"], c["secret"] and len(c["secret"]) // 2)
        random.seed("before-" + c["file"])
        item = [(beat, c["num"], og.root_seed_of(c["root_seed"]))]
        if "error" in c:
            kind, text = c["error"][1:].split(": ", 1)
            with pytest.raises(Exception) as ex:
                O.OneHash.generate_challenges_many(item, chain=chain)
            assert type(ex.value).__name__ == kind and (kind != "HeartbeatError" or str(ex.value) == text), key
        else:
            O.OneHash.generate_challenges_many(item, chain=chain)
            assert og.matches(c["blocks"], [x.block for x in beat.challenges]), key
            assert og.matches(c["seeds"], [x.seed.hex() for x in beat.challenges]), key
            assert og.matches(c["responses"], [x.response.hex() for x in beat.challenges]), key
        assert random.random() == c["next_random"], key


def test_generate_challenges_public_call(O, paths):
    """generate_challenges itself (the runtime's own choice of chain)."""
    c = next(c for c in G["generate"] if c["num"] == 300 and c["file"] == "det100003" and "error" not in c)
    beat = O.OneHash(paths[c["file"]], bytes.fromhex(c["secret"]))
    beat.generate_challenges(c["num"], og.root_seed_of(c["root_seed"]))
    assert random.random() == c["next_random"]
    assert og.matches(c["responses"], [x.response.hex() for x in beat.challenges])
    assert beat.check_answer(beat.challenges[7].response) and len(beat.challenges) == 299


def test_unforced_calls_cross_over_at_the_measured_job_count(O, paths, monkeypatch):
    """With neither path forced a call goes to the GPU from
    hb_onehash_device_min_jobs() eligible jobs, and stays on the host below;
    both give the recorded responses."""
    from heartbeat_amd import _native
    monkeypatch.delenv("HB_ONEHASH_DEVICE")
    floor = _native.lib().hb_onehash_device_min_jobs()
    assert 1 < floor <= 300
    c = next(c for c in G["generate"] if c["num"] == 300 and c["file"] == "test.txt" and "error" not in c)
    beat = O.OneHash(paths[c["file"]], bytes.fromhex(c["secret"]))
    calls = []
    real_meet, real_gen = O.OneHash._gpu_meet, O.OneHash._gpu_generate
    monkeypatch.setattr(O.OneHash, "_gpu_meet", staticmethod(lambda p: calls.append(("meet", len(p))) or real_meet(p)))
    monkeypatch.setattr(O.OneHash, "_gpu_generate",
                        staticmethod(lambda p, chain=None: calls.append(("gen", p[0][1])) or real_gen(p, chain)))
    beat.generate_challenges(300, og.root_seed_of(c["root_seed"]))
    assert og.matches(c["responses"], [x.response.hex() for x in beat.challenges])
    want = [x.response for x in beat.challenges]
    assert beat.meet_challenges(beat.challenges[:floor]) == want[:floor]
    assert calls == [("gen", 300), ("meet", floor)]
    assert beat.meet_challenges(beat.challenges[:floor - 1]) == want[:floor - 1]
    beat.generate_challenges(floor - 1, og.root_seed_of(c["root_seed"]))
    assert [x.response for x in beat.challenges] == want[:floor - 1]
    assert beat.meet_challenge(beat.challenges[0]) == want[0]
    assert len(calls) == 2   # all three stayed on the host


def test_generate_many_72_files(O, paths):
    """72 files x 3 challenges in one call -- more than one wave on the chain
    kernel, secrets of 0 to 200 bytes side by side (above 87 the host walks
    that file's chain) -- with the chains forced onto the host and onto the
    GPU: both are the reference's recorded results."""
    cases = [c for c in G["generate"] if c["num"] == 3 and "error" not in c]
    cases = [cases[k % len(cases)] for k in range(72)]
    assert {len(c["secret"]) // 2 for c in cases} >= {0, 8, 23, 24, 87, 88, 200}
    for chain in ("host", "device"):
        beats = [O.OneHash(paths[c["file"]], bytes.fromhex(c["secret"])) for c in cases]
        O.OneHash.generate_challenges_many(
            [(b, 3, og.root_seed_of(c["root_seed"])) for b, c in zip(beats, cases)], chain=chain)
        assert random.random() == cases[-1]["next_random"]
        for b, c in zip(beats, cases):
            got = [(x.block, x.seed.hex(), x.response.hex()) for x in b.challenges]
            assert got == list(zip(c["blocks"]["all"], c["seeds"]["all"], c["responses"]["all"])), (chain, c["file"])


def test_large_host_file_is_gathered(O, tmp_path):
    """A 9 MiB host file with 200 challenges lies above the upload threshold
    max(2 * 200 * 1024, 8 MiB): only the jobs' segments go up.  Blocks from
    pick_blocks and on both sides of the wrap and of the short read."""
    data = splitmix_bytes(11, 0, (9 << 20) + 7)
    p = tmp_path / "big.bin"
    p.write_bytes(data)
    fs = len(data)
    beat = O.OneHash(str(p), b"secret")
    edge = [0, 1, fs - 1025, fs - 1024, fs - 1023, fs - 513, fs - 512, fs - 511, fs - 2, fs - 1]
    blocks = edge + beat.pick_blocks(200 - len(edge), b"root")
    seeds = beat.generate_seeds(200, b"root", b"secret")
    got = beat.meet_challenges([O.Challenge(b, s) for b, s in zip(blocks, seeds)])
    assert got == [_expect(data, b, s) for b, s in zip(blocks, seeds)]
    beat.generate_challenges(200, b"root")
    want_blocks = beat.pick_blocks(200, b"root")
    assert [(c.block, c.seed) for c in beat.challenges] == list(zip(want_blocks, seeds))
    assert [c.response for c in beat.challenges] == [_expect(data, b, s) for b, s in zip(want_blocks, seeds)]


def test_bad_descriptors_are_refused_before_any_launch(O):
    """The raw ABI: every bad descriptor returns HB_EINVAL with a message, and
    the context still serves a good call afterwards."""
    from heartbeat_amd import _native
    ctx, L = _native.context(), _native.lib()
    data = np.frombuffer(og.file_bytes("det1000"), dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    files = (_native.OneHashFile * 1)()
    files[0].data, files[0].len = data.ctypes.data, len(data)

    def meet(file=0, block=5, seed_len=32, flags=0, files_p=files, out_p=out.ctypes.data):
        rec = np.zeros(2, dtype=_native.ONEHASH_JOB_DTYPE)
        rec["file"], rec["block"], rec["seed_len"] = [0, file], [7, block], [32, seed_len]
        return L.hb_onehash_meet_many(ctx.h, files_p, 1, rec.ctypes.data, 2, out_p, flags)

    for kw, text in (({"file": 1}, "no file"), ({"block": 1000}, "outside the file"),
                     ({"block": (1 << 64) - 1}, "outside the file"), ({"seed_len": 65}, "seed longer"),
                     ({"flags": 2}, "unsupported flags"), ({"out_p": None}, "NULL"), ({"files_p": None}, "NULL")):
        assert meet(**kw) == -1, kw
        assert text in L.hb_last_error(ctx.h).decode(), kw
    assert meet() == 0
    want = hashlib.sha256(data.tobytes()[5:105] + bytes(32)).digest()
    assert out.tobytes()[32:] == want

    s0, blocks = hashlib.sha256(b"r").digest(), np.array([5, 999], dtype=np.uint64)
    seeds, resp = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)

    def gen(flags=0, len_=len(data), blocks_p=blocks.ctypes.data, s0_p=s0, seeds_p=seeds.ctypes.data):
        d = (_native.OneHashGenDesc * 1)()
        d[0].data, d[0].len, d[0].s0, d[0].secret, d[0].secret_len = data.ctypes.data, len_, s0_p, b"sec", 3
        d[0].num, d[0].blocks = 2, blocks_p
        return L.hb_onehash_generate_many(ctx.h, d, 1, seeds_p, resp.ctypes.data, flags)

    for kw, text in (({"len_": 999}, "outside the file"), ({"flags": 64 | 128}, "unsupported flags"),
                     ({"flags": 2}, "unsupported flags"), ({"blocks_p": None}, "NULL"), ({"s0_p": None}, "NULL"),
                     ({"seeds_p": None}, "NULL")):
        assert gen(**kw) == -1, kw
        assert text in L.hb_last_error(ctx.h).decode(), kw
    assert gen() == 0
    s1 = hashlib.sha256(s0 + b"sec").digest()
    assert seeds.tobytes() == s0 + s1
    assert resp.tobytes() == _expect(data.tobytes(), 5, s0) + _expect(data.tobytes(), 999, s1)
