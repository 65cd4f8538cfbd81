"""The OneHash scheme's surface: heartbeat.OneHash re-exports
heartbeat_amd.OneHash under the reference's module paths, ``import heartbeat``
does not import it (as in the reference), the ctypes signatures stand beside
the header, and the reference's unit-test scenarios
(tests/tests_unit_onehash.py), restated, hold on the host path."""
import ctypes
import hashlib
import io
import os
import pickle
import random
import subprocess
import sys
from decimal import Decimal

import pytest

from conftest import GOLDEN, ROOT

TEST_TXT = os.path.join(GOLDEN, "files", "test.txt")


def test_alias_package():
    import heartbeat.OneHash
    import heartbeat_amd.OneHash
    assert heartbeat.OneHash.OneHash is heartbeat_amd.OneHash.OneHash
    assert heartbeat.OneHash.Challenge is heartbeat_amd.OneHash.Challenge
    from heartbeat.OneHash import OneHash, Challenge   # the reference's tests' import
    from heartbeat.OneHash.OneHash import OneHash as O2
    assert O2 is OneHash and OneHash.__module__ == "heartbeat.OneHash.OneHash"
    c = Challenge(5, b"seed")
    c.response = b"r"
    assert pickle.dumps(c).find(b"heartbeat.OneHash.OneHash") > 0
    d = pickle.loads(pickle.dumps(c))
    assert type(d) is Challenge and (d.block, d.seed, d.response) == (5, b"seed", b"r")
    w = c.without_answer
    assert not hasattr(w, "response") and (w.block, w.seed) == (5, b"seed") and c.response == b"r"


def test_import_heartbeat_leaves_onehash_and_the_library_alone():
    code = (
        "import sys\n"
        "import heartbeat\n"
        "assert 'heartbeat.OneHash' not in sys.modules and not hasattr(heartbeat, 'OneHash')\n"
        "from heartbeat.OneHash import OneHash, Challenge\n"
        "for name in ('generate_challenges', 'meet_challenge', 'generate_seeds', 'pick_blocks', 'check_answer',\n"
        "             'delete_challenge', 'random_challenge', 'meet_challenges', 'meet_many',\n"
        "             'generate_challenges_many', 'from_device'):\n"
        "    assert callable(getattr(OneHash, name)), name\n"
        "assert isinstance(OneHash.challenges_size, property) and isinstance(Challenge.without_answer, property)\n"
        "import os\n"
        "os.environ['HB_ONEHASH_HOST'] = '1'\n"
        "beat = OneHash(%r, b'mysecret')\n"
        "beat.generate_challenges(300, b'root')\n"
        "assert beat.meet_challenges(beat.challenges) == [c.response for c in beat.challenges]\n"
        "from heartbeat_amd import _native\n"
        "assert _native._lib is None, 'the import or the host path loaded libhbswizzle.so'\n"
        "print('ok')\n" % TEST_TXT)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_native_binding_lists_the_onehash_calls():
    from heartbeat_amd import _native
    import numpy as np
    sig = {s[0]: s for s in _native.SIGNATURES}
    c = ctypes
    assert sig["hb_onehash_generate_many"][1:] == (c.c_int, [c.c_void_p, c.POINTER(_native.OneHashGenDesc),
                                                             c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32])
    assert sig["hb_onehash_meet_many"][1:] == (c.c_int, [c.c_void_p, c.POINTER(_native.OneHashFile), c.c_uint64,
                                                         c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32])
    assert [f[0] for f in _native.OneHashGenDesc._fields_] == ["data", "len", "s0", "secret", "secret_len", "num",
                                                               "blocks"]
    assert ctypes.sizeof(_native.OneHashGenDesc) == 7 * 8 and ctypes.sizeof(_native.OneHashFile) == 2 * 8
    assert ctypes.sizeof(_native.OneHashJob) == 88 == np.dtype(_native.ONEHASH_JOB_DTYPE).itemsize
    dt = np.dtype(_native.ONEHASH_JOB_DTYPE)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [
        (f[0], getattr(_native.OneHashJob, f[0]).offset) for f in _native.OneHashJob._fields_]
    with open(os.path.join(ROOT, "include", "hbswizzle.h")) as fh:
        header = " ".join(fh.read().split())
    assert ("int hb_onehash_generate_many(hb_ctx *ctx, const hb_onehash_gen_desc *files, uint64_t nfiles, "
            "uint8_t *seeds_out, uint8_t *responses_out, uint32_t flags);") in header
    assert ("int hb_onehash_meet_many(hb_ctx *ctx, const hb_onehash_file *files, uint64_t nfiles, "
            "const hb_onehash_job *jobs, uint64_t njobs, uint8_t *responses_out, uint32_t flags);") in header
    assert "uint64_t hb_onehash_device_min_jobs(void);" in header
    assert "#define HB_ONEHASH_CHAIN_HOST %du" % _native.HB_ONEHASH_CHAIN_HOST in header
    assert "#define HB_ONEHASH_CHAIN_DEVICE %du" % _native.HB_ONEHASH_CHAIN_DEVICE in header
    assert "#define HB_ONEHASH_MAX_SEED_LEN %du" % _native.HB_ONEHASH_MAX_SEED_LEN in header


# ---------------------------------------------------------------- the reference's unit-test scenarios
@pytest.fixture
def hb(monkeypatch):
    monkeypatch.setenv("HB_ONEHASH_HOST", "1")
    from heartbeat.OneHash import OneHash
    return OneHash(TEST_TXT, b"mysecret")


def test_challenge_init():
    from heartbeat.OneHash import Challenge
    c = Challenge([], [])
    assert c.block == [] and c.seed == [] and c.response is None


def test_initialization(hb):
    from heartbeat.OneHash import OneHash
    assert hb.file_size == os.path.getsize(TEST_TXT)
    assert isinstance(hb.file_object, io.BufferedReader)
    assert isinstance(hb.challenges, list) and len(hb.challenges) == 0
    assert len(OneHash(TEST_TXT, os.urandom(32)).secret) == 32


def test_initialization_fail():
    from heartbeat.exc import HeartbeatError
    from heartbeat.OneHash import OneHash
    with pytest.raises(HeartbeatError) as ex:
        OneHash('does/not/exist')
    assert ex.value.message == 'does/not/exist not found'


def test_generate_seeds(hb):
    from heartbeat.exc import HeartbeatError
    digest = hashlib.sha256(b"24 bytes").digest()
    for root in (bytes(123), Decimal(0.25) + 5, hashlib.sha256(b"x"), digest, digest.hex()):
        seeds = hb.generate_seeds(4, root, hb.secret)
        assert len(seeds) == 4 and all(isinstance(s, bytes) for s in seeds)
    assert hb.generate_seeds(5, digest, hb.secret) == hb.generate_seeds(5, digest, hb.secret)
    with pytest.raises(HeartbeatError) as ex:
        hb.generate_seeds(-1, 7, hb.secret)
    assert ex.value.message == '-1 is not greater than 0'
    with pytest.raises(HeartbeatError) as ex:
        hb.generate_seeds(4, digest, None)
    assert ex.value.message == 'secret can not be of type NoneType'


def test_pick_blocks(hb):
    from heartbeat.exc import HeartbeatError
    digest = hashlib.sha256(b"24 bytes").digest()
    for root in (4711, 5.25, digest, digest.hex()):
        blocks = hb.pick_blocks(4, root)
        assert len(blocks) == 4 and all(isinstance(b, int) and 0 <= b < hb.file_size for b in blocks)
    assert hb.pick_blocks(5, digest) == hb.pick_blocks(5, digest)
    got = hb.pick_blocks(3, digest)
    random.seed(digest)
    assert got == [random.randint(0, hb.file_size - 1) for _ in range(3)]
    with pytest.raises(HeartbeatError) as ex:
        hb.pick_blocks(-1, 7)
    assert ex.value.message == '-1 is not greater than 0'


def test_meet_challenge_and_near_eof(hb):
    from heartbeat.OneHash import Challenge
    with open(TEST_TXT, "rb") as fh:
        data = fh.read()
    chunk = min(1024, hb.file_size // 10)
    seed = os.urandom(32)
    assert hb.meet_challenge(Challenge(0, seed)) == hashlib.sha256(data[:chunk] + seed).digest()
    block = 3100
    assert block > hb.file_size - chunk
    end = block - (hb.file_size - chunk)
    want = hashlib.sha256(data[block:block + end] + data[:chunk - end] + seed).digest()
    assert hb.meet_challenge(Challenge(block, seed)) == want


def test_generate_check_delete_random(hb):
    from heartbeat.OneHash import Challenge
    digest = hashlib.sha256(b"root").digest()
    hb.generate_challenges(7, digest)
    assert all(isinstance(c, Challenge) for c in hb.challenges)
    seeds, blocks = hb.generate_seeds(7, digest, hb.secret), hb.pick_blocks(7, digest)
    for c, s, b in zip(hb.challenges, seeds, blocks):
        assert (c.seed, c.block) == (s, b) and hb.meet_challenge(c) == c.response
    assert hb.challenges_size == sys.getsizeof(hb.challenges)
    rc = hb.random_challenge()
    assert isinstance(rc, Challenge) and any(c.block == rc.block for c in hb.challenges)
    assert hb.check_answer("test value that doesn't matter.  ;)") is False
    assert hb.delete_challenge(b"invalid hash that doesn't matter") is False and len(hb.challenges) == 7
    assert hb.delete_challenge(hb.challenges[2].response) is True and len(hb.challenges) == 6
    value = hb.challenges[0].response
    assert hb.check_answer(value) is True and len(hb.challenges) == 5
    assert hb.check_answer(value) is False   # spent
