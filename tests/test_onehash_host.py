"""heartbeat_amd.OneHash on its forced host path (HB_ONEHASH_HOST=1) against
the reference's recorded outputs (tests/golden/onehash_cases.json): every
response, the results and exception types of the blocks only a foreign
challenger sends, every generate_challenges case and the module-level
generator's next draw after it.  No GPU is needed (that the host path does not
load the native library either: tests/test_onehash_import_surface.py)."""
import random

import pytest

import onehash_golden as og
from conftest import load_golden

G = load_golden("onehash_cases.json")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("HB_ONEHASH_HOST", "1")
    monkeypatch.delenv("HB_ONEHASH_DEVICE", raising=False)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return og.write_files(tmp_path_factory.mktemp("onehash_files"), G["files"])


def outcome(fn):
    """The result, or the exception as the golden file records it."""
    try:
        return fn()
    except Exception as e:
        return "!%s: %s" % (type(e).__name__, e)


def same(got, want):
    """Results equal; exceptions of one type, and of one text where the text
    is the scheme's own (HeartbeatError) and not the interpreter's."""
    if want.startswith("!") and isinstance(got, str) and got.startswith("!"):
        kind = want.split(":")[0]
        return got == want if kind == "!HeartbeatError" else got.split(":")[0] == kind
    return got == want


def test_meet_challenge_every_golden_case(paths):
    from heartbeat_amd.OneHash import Challenge, OneHash
    n = 0
    for name in G["files"]:
        beat = OneHash(paths[name])   # no secret: it still answers
        assert beat.file_size == G["files"][name]["len"]
        for c in (c for c in G["meet"] if c["file"] == name):
            for sl, want in c["answers"].items():
                got = outcome(lambda: beat.meet_challenge(Challenge(c["block"], og.seed_of(int(sl)))).hex())
                assert same(got, want), (name, c["block"], sl, got, want)
                n += 1
    assert n > 1300


def test_out_of_range_blocks(paths):
    """What the issue pins for a foreign challenger's blocks."""
    import hashlib
    from heartbeat_amd.OneHash import Challenge, OneHash
    beat = OneHash(paths["det1000"])
    data, seed = og.file_bytes("det1000"), b"s" * 32
    assert beat.meet_challenge(Challenge(1000, seed)) == hashlib.sha256(seed).digest()
    assert beat.meet_challenge(Challenge(1001, seed)) == hashlib.sha256(data + seed).digest()
    with pytest.raises(ValueError):
        beat.meet_challenge(Challenge(1002, seed))
    with pytest.raises(OSError):
        beat.meet_challenge(Challenge(-1, seed))


def test_generate_challenges_every_golden_case(paths):
    from heartbeat_amd.OneHash import OneHash
    for c in G["generate"]:
        secret = None if c["secret"] is None else bytes.fromhex(c["secret"])
        beat = OneHash(paths[c["file"]], secret)
        random.seed("before-" + c["file"])
        got = outcome(lambda: beat.generate_challenges(c["num"], og.root_seed_of(c["root_seed"])))
        key = (c["file"], c["num"], c["root_seed"]["t"], c["secret"] and len(c["secret"]) // 2)
        assert random.random() == c["next_random"], key
        if "error" in c:
            assert same(got, c["error"]), (key, got)
            assert beat.challenges == []
            continue
        assert got is None and len(beat.challenges) == c["num"], key
        assert og.matches(c["blocks"], [x.block for x in beat.challenges]), key
        assert og.matches(c["seeds"], [x.seed.hex() for x in beat.challenges]), key
        assert og.matches(c["responses"], [x.response.hex() for x in beat.challenges]), key


def test_batches_equal_loops_on_the_host(paths):
    """meet_challenges, meet_many and generate_challenges_many return what a
    loop of the single calls returns, and leave the generator where it does."""
    from heartbeat_amd.OneHash import Challenge, OneHash
    names = ["det100", "det10241", "test.txt"]
    items = [(OneHash(paths[n], b"secret-%d" % k), 7 + k, b"root%d" % k) for k, n in enumerate(names)]
    loop = [OneHash(paths[n], b"secret-%d" % k) for k, n in enumerate(names)]
    for b, (_, num, root) in zip(loop, items):
        b.generate_challenges(num, root)
    after_loop = random.random()
    OneHash.generate_challenges_many(items)
    assert random.random() == after_loop
    for b, (m, _, _) in zip(loop, items):
        assert [(c.block, c.seed, c.response) for c in m.challenges] == \
            [(c.block, c.seed, c.response) for c in b.challenges]
    pairs = [(b, c.without_answer) for b in loop for c in b.challenges] + [(loop[0], Challenge(100, b"x" * 70))]
    assert OneHash.meet_many(pairs) == [b.meet_challenge(c) for b, c in pairs]
    assert loop[1].meet_challenges(loop[1].challenges) == [c.response for c in loop[1].challenges]
    # an item the reference fails on: the items before it are done, then it raises
    a, b = OneHash(paths["det100"], b"s"), OneHash(paths["det100"], None)
    with pytest.raises(Exception, match="secret can not be of type NoneType"):
        OneHash.generate_challenges_many([(a, 2, b"r"), (b, 2, b"r"), (a, 5, b"r")])
    assert len(a.challenges) == 2 and b.challenges == []
