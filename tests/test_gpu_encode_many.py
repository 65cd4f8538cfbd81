"""GPU parity of the batched encode (hb_encode_many, PySwizzle.encode_many):
many small files, each under its own f_key and alpha_key, in one PRF launch
and one MAC launch (hb_batch.hpp; hb_runtime.cpp encode_many_impl).

For every file the batch's tags == hb_encode's == the CPU oracle's, and the
batch's tries == the sum of the single calls' tries, over

* the block-boundary lengths (0, 1, ss-1, ss, C-1, C, C+1, one full wave-job,
  one block more, a short sector followed by zero sectors),
* every limb count and AES key size, S = 1, sectors without 16-byte loads,
* distinct keys per file, more wave-jobs than the chip has wave positions,
* alpha over several wave-jobs and S above the sector-parallel MAC's width,
* device-resident files and tags at odd addresses,
* launch splitting and the fall-through of a large file ($HB_TEST_BATCH_BLOCKS),
* the context afterwards (prove, verify, a plain encode), unsupported flags.

Reference: a caller's loop over PySwizzle.py:279-311."""
import ctypes
import importlib
import io
import random

import numpy as np
import pytest

from test_gpu_parity import P256, DevBuf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


@pytest.fixture(scope="module")
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


def _prime(bits, seed):
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    rng = random.Random(seed)
    while True:
        p = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if pys._is_probable_prime(p):
            return p


def _nblocks(p, S, n):
    return n // ((p.bit_length() // 8) * S) + 1


def _inputs(seed, lengths, klen):
    """Seeded file bytes and key pairs, one per length."""
    rng = np.random.default_rng(seed)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]
    keys = [(rng.integers(0, 256, klen, dtype=np.uint8).tobytes(), rng.integers(0, 256, klen, dtype=np.uint8).tobytes())
            for _ in lengths]
    return datas, keys


def encode_many(nat, p, S, keys, datas, flags=0, data_ptrs=None, tag_ptrs=None, fill=None):
    """hb_encode_many: (rc, [tag bytes per file] for host tags, tries).  Host
    buffers unless data_ptrs / tag_ptrs give device addresses."""
    ctx = nat.context()
    n = len(datas)
    w = nat.width_of(p)
    descs = (nat.FileDesc * max(n, 1))()
    arrs, outs = [], []
    for i in range(n):
        a = np.frombuffer(datas[i], dtype=np.uint8)
        arrs.append(a)
        out = np.empty(_nblocks(p, S, len(datas[i])) * w, dtype=np.uint8)
        if fill is not None:
            out[:] = fill
        outs.append(out)
        descs[i].f_key, descs[i].alpha_key = keys[i]
        if data_ptrs is not None:
            descs[i].data = data_ptrs[i]
        else:
            descs[i].data = a.ctypes.data if len(a) else None
        descs[i].len = len(datas[i])
        descs[i].tags = tag_ptrs[i] if tag_ptrs is not None else out.ctypes.data
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        rc = nat.lib().hb_encode_many(ctx.h, pb, len(pb), S, len(keys[0][0]) if n else 32, descs, n, flags,
                                      ctypes.byref(tries))
    return rc, [o.tobytes() for o in outs], tries.value


def encode_single(nat, p, S, fk, ak, data):
    """One host-buffer hb_encode of a whole file: (tag bytes, tries)."""
    ctx = nat.context()
    w = nat.width_of(p)
    nb = _nblocks(p, S, len(data))
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(nb * w, dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), 0, a.ctypes.data if len(a) else None,
                                      len(data), nb, out.ctypes.data, 0, ctypes.byref(tries)))
    return out.tobytes(), tries.value


def oracle_raw(oracle, p, S, fk, ak, data, w):
    return b"".join(t.to_bytes(w, "big") for t in oracle.encode(p, S, fk, ak, data))


def check_batch(nat, oracle, p, S, lengths, klen, seed):
    """Batch == single == oracle for every file, tries == the singles' sum."""
    datas, keys = _inputs(seed, lengths, klen)
    w = nat.width_of(p)
    rc, got, tries = encode_many(nat, p, S, keys, datas)
    assert rc == 0, nat.lib().hb_last_error(nat.context().h)
    total = 0
    for i, d in enumerate(datas):
        one, t = encode_single(nat, p, S, keys[i][0], keys[i][1], d)
        total += t
        assert got[i] == one, (i, len(d))
        assert got[i] == oracle_raw(oracle, p, S, keys[i][0], keys[i][1], d, w), (i, len(d))
    assert tries == total
    return datas, keys, got


# ------------------------------------------------------------------ 1: boundaries
S1, SS1, C1 = 16, 32, 512


@pytest.fixture(scope="module")
def batch1(nat, oracle):
    """Test 1's batch, checked once; (datas, keys, tag bytes per file)."""
    rng = np.random.default_rng(101)
    lengths = [0, 1, SS1 - 1, SS1, C1 - 1, C1, C1 + 1, 15 * C1 + 7, 16 * C1, 16 * C1 + SS1 + 3, 33 * C1 - 1]
    lengths += [int(x) for x in rng.integers(0, 64 << 10, 25)]
    return check_batch(nat, oracle, P256, S1, lengths, 32, 1)


def test_batch_equals_single_and_oracle(batch1):
    datas, keys, got = batch1
    assert len(got) == 36


# ------------------------------------------------------------------ 2: limbs, key sizes
@pytest.mark.parametrize("bits,S,klen", [
    (16, 3, 16),       # 2-byte sectors, AES-128
    (256, 1, 24),      # S = 1: one lane per block, AES-192
    (384, 5, 32),      # 48-byte sectors: no 16-byte loads
    (512, 16, 32),
    (1024, 10, 32),    # PySwizzle's defaults
    (2048, 4, 32),     # 64 limbs
])
def test_limb_counts_and_key_sizes(nat, oracle, bits, S, klen):
    p = P256 if bits == 256 else _prime(bits, 7 * bits + S)
    ss = p.bit_length() // 8
    C = ss * S
    rnd = int(np.random.default_rng(bits).integers(0, 40 * C))
    check_batch(nat, oracle, p, S, [0, ss - 1, C, 17 * C + 5, rnd], klen, bits + S)


# ------------------------------------------------------------------ 3: keys stay with their file
def test_keys_stay_with_their_file(nat, oracle):
    data = np.random.default_rng(3).integers(0, 256, 3 * C1 + 1, dtype=np.uint8).tobytes()
    _, keys = _inputs(33, [0] * 32, 32)
    keys.append(keys[0])
    rc, got, _ = encode_many(nat, P256, S1, keys, [data] * 33)
    assert rc == 0
    w = nat.width_of(P256)
    for i in range(33):
        assert got[i] == oracle_raw(oracle, P256, S1, keys[i][0], keys[i][1], data, w), i
    assert got[0] == got[32]
    assert len(set(got[:32])) == 32


# ------------------------------------------------------------------ 4: more wave-jobs than positions
def test_more_wave_jobs_than_wave_positions(nat, oracle):
    rng = np.random.default_rng(4)
    lengths = [int(x) for x in rng.integers(0, C1, 5000)]
    datas, keys = _inputs(44, lengths, 32)
    rc, got, tries = encode_many(nat, P256, S1, keys, datas)
    assert rc == 0
    assert tries >= 5000
    w = nat.width_of(P256)
    for i in range(5000):
        assert got[i] == oracle_raw(oracle, P256, S1, keys[i][0], keys[i][1], datas[i], w), i


# ------------------------------------------------------------------ 5: wide alpha, S above the split MAC
@pytest.mark.parametrize("S", [40, 300])
def test_many_sectors(nat, oracle, S):
    C = 32 * S
    check_batch(nat, oracle, P256, S, [0, C - 1, C, 5 * C + 9], 32, S)


# ------------------------------------------------------------------ 6: device-resident
def test_device_resident_odd_offsets(nat, batch1):
    datas, keys, want = batch1
    datas, keys, want = datas[:16], keys[:16], want[:16]
    w = nat.width_of(P256)
    doffs, toffs, d, t = [], [], 1, 1
    for x in datas:
        doffs.append(d)
        toffs.append(t)
        d = (d + len(x) + 2) | 1
        t = (t + _nblocks(P256, S1, len(x)) * w + 2) | 1
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    try:
        for x, o in zip(datas, doffs):
            dbuf.upload(x, o)
        rc, _, tries = encode_many(nat, P256, S1, keys, datas, flags=3, data_ptrs=[dbuf.p + o for o in doffs],
                                   tag_ptrs=[tbuf.p + o for o in toffs])
        assert rc == 0
        raw = tbuf.download()
    finally:
        dbuf.free()
        tbuf.free()
    for i, x in enumerate(datas):
        n = _nblocks(P256, S1, len(x)) * w
        assert raw[toffs[i]:toffs[i] + n] == want[i], i


# ------------------------------------------------------------------ 7: splitting, fall-through
def test_launch_splitting(nat, batch1, monkeypatch):
    datas, keys, want = batch1
    total = sum(_nblocks(P256, S1, len(x)) for x in datas)
    biggest = max(_nblocks(P256, S1, len(x)) for x in datas)
    cap = max(total // 3, biggest)
    assert 3 * cap <= total + 2 and biggest <= cap   # at least three groups, no file falls through
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", str(cap))
    try:
        rc, got, _ = encode_many(nat, P256, S1, keys, datas)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0
    assert got == want
    assert nat.context().last_kernel_ms()[1] >= 6   # two launches per group


def test_large_file_falls_through(nat, oracle, monkeypatch):
    lengths = [5 * C1 + 3, 3 << 20, 2 * C1]
    datas, keys = _inputs(77, lengths, 32)
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", "4096")   # the 3 MiB file has 6,145 blocks
    try:
        rc, got, tries = encode_many(nat, P256, S1, keys, datas)
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0
    w = nat.width_of(P256)
    for i, x in enumerate(datas):
        want = b"".join(t.to_bytes(w, "big") for t in oracle.encode(P256, S1, keys[i][0], keys[i][1], x, nthreads=8))
        assert got[i] == want, i
    assert tries >= sum(_nblocks(P256, S1, n) for n in lengths)


# ------------------------------------------------------------------ 8: the context afterwards
def test_context_left_clean(nat, oracle, pys, tmp_path):
    rng = np.random.default_rng(8)
    datas = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 20000, 10)]
    files = [io.BytesIO(x) for x in datas[:8]]
    for k in (8, 9):
        path = tmp_path / ("f%d.bin" % k)
        path.write_bytes(datas[k])
        files.append(open(str(path), "rb"))
    beat = pys.PySwizzle(S1, b"k" * 32, P256)
    try:
        res = beat.encode_many(files)
    finally:
        for f in files[8:]:
            f.close()
    assert len(res) == 10
    pub = beat.get_public()
    for x, (tag, state) in zip(datas, res):
        assert len(tag) == _nblocks(P256, S1, len(x))
        chal = beat.gen_challenge(state)
        assert beat.verify(pub.prove(io.BytesIO(x), chal, tag), chal, state)
        bad = bytearray(x)
        bad[len(bad) // 2] ^= 1
        # 64 draws per block: the flipped byte's block is missed by all of
        # them with probability (1 - 1/n)^(64 n) < e^-64
        chal = pys.Challenge(64 * len(tag), P256, bytes([len(tag) % 251]) * 32)
        assert beat.verify(pub.prove(io.BytesIO(x), chal, tag), chal, state)
        assert not beat.verify(pub.prove(io.BytesIO(bytes(bad)), chal, tag), chal, state)
    tag, state = beat.encode(io.BytesIO(datas[0]))
    state.decrypt(beat.key)
    assert tag.sigma == oracle.encode(P256, S1, state.f_key, state.alpha_key, datas[0])


# ------------------------------------------------------------------ 9: unsupported flags
@pytest.mark.parametrize("flag", ["HB_PRF_CXX", "HB_ASYNC", "HB_ENCODE_SINGLE_PASS"])
def test_unsupported_flags(nat, flag):
    datas, keys = _inputs(9, [100, 1000], 32)
    rc, got, _ = encode_many(nat, P256, S1, keys, datas, flags=getattr(nat, flag), fill=0xA5)
    assert rc == nat.HB_EUNSUPPORTED
    assert all(set(g) == {0xA5} for g in got)


def test_empty_batch(nat):
    rc, got, tries = encode_many(nat, P256, S1, [], [])
    assert rc == 0 and got == [] and tries == 0
