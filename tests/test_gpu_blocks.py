"""GPU parity of the listed-block encode (hb_encode_blocks,
hb_encode_blocks_many): tags[k] of a file are the bytes hb_encode writes for
block_base = indices[k], the k-th packed block and nblocks = 1.

Reference throughout: oracle.encode(..., block_base=i, nblocks=1) -- the body
of heartbeat/PySwizzle/PySwizzle.py:296-309 for one i -- and, where the indices
lie inside a file, hb_encode of the whole file read at the listed indices.

* the golden cases' blocks in reversed order against the recorded tags,
* indices up to 2^64 - 1, repeated and unsorted, in one call,
* list sizes around the wave-job (16) and the wave (64), a forced split,
* every length of the last listed block,
* limb counts, key lengths, S = 1 / 10 / above the sector-parallel MAC,
* batches of files with their own keys, an empty list among them, tries,
* device-resident data and tags at odd addresses,
* unsupported flags and bad descriptors, and the context afterwards."""
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


def _prime(bits, seed):
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    rng = random.Random(seed)
    while True:
        p = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if pys._is_probable_prime(p):
            return p


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _keys(seed, n, klen=32):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, klen, dtype=np.uint8).tobytes(), rng.integers(0, 256, klen, dtype=np.uint8).tobytes())
            for _ in range(n)]


def blocks_many(nat, p, S, files, flags=0, fill=None, data_ptrs=None, tag_ptrs=None, klen=None):
    """hb_encode_blocks_many over files = [(f_key, alpha_key, indices, packed
    bytes)]: (rc, [tag bytes per file] for host tags, tries)."""
    ctx = nat.context()
    n = len(files)
    w = nat.width_of(p)
    descs = (nat.BlocksDesc * max(n, 1))()
    keep, outs = [], []
    for i, (fk, ak, indices, data) in enumerate(files):
        idx = np.array(indices, dtype=np.uint64)
        a = np.frombuffer(data, dtype=np.uint8)
        out = np.empty(len(idx) * w, dtype=np.uint8)
        if fill is not None:
            out[:] = fill
        keep.append((idx, a))
        outs.append(out)
        d = descs[i]
        d.f_key, d.alpha_key = fk, ak
        d.indices, d.nblocks = (idx.ctypes.data if len(idx) else None), len(idx)
        d.data = data_ptrs[i] if data_ptrs is not None else (a.ctypes.data if len(a) else None)
        d.len = len(data)
        d.tags = tag_ptrs[i] if tag_ptrs is not None else (out.ctypes.data if len(idx) else None)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    if klen is None:
        klen = len(files[0][0]) if n else 32
    with ctx.lock:
        rc = nat.lib().hb_encode_blocks_many(ctx.h, pb, len(pb), S, klen, descs, n, flags, ctypes.byref(tries))
    return rc, [o.tobytes() for o in outs], tries.value


def blocks_one(nat, p, S, fk, ak, indices, data, flags=0):
    """hb_encode_blocks: (rc, tag bytes, tries)."""
    ctx = nat.context()
    w = nat.width_of(p)
    idx = np.array(indices, dtype=np.uint64)
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(len(idx) * w, dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        rc = nat.lib().hb_encode_blocks(ctx.h, pb, len(pb), S, fk, ak, len(fk), idx.ctypes.data if len(idx) else None,
                                        len(idx), a.ctypes.data if len(a) else None, len(data),
                                        out.ctypes.data if len(idx) else None, flags, ctypes.byref(tries))
    return rc, out.tobytes(), tries.value


def single_block(nat, p, S, fk, ak, index, data):
    """hb_encode of one block at block_base = index: (tag bytes, tries)."""
    ctx = nat.context()
    w = nat.width_of(p)
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(w, dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), index, a.ctypes.data if len(a) else None,
                                      len(data), 1, out.ctypes.data, 0, ctypes.byref(tries)))
    return out.tobytes(), tries.value


def whole_file(nat, p, S, fk, ak, data):
    """hb_encode of a whole file: its tag bytes."""
    ctx = nat.context()
    w = nat.width_of(p)
    nb = len(data) // ((p.bit_length() // 8) * S) + 1
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(nb * w, dtype=np.uint8)
    pb = nat.be(p)
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), S, fk, ak, len(fk), 0, a.ctypes.data if len(a) else None,
                                      len(data), nb, out.ctypes.data, 0, None))
    return out.tobytes()


def ref_tags(oracle, p, S, fk, ak, indices, data):
    """The reference: one oracle.encode(block_base=i, nblocks=1) per listed block."""
    w = (p.bit_length() + 7) // 8
    C = (p.bit_length() // 8) * S
    return b"".join(oracle.encode(p, S, fk, ak, data[k * C:(k + 1) * C], block_base=int(i), nblocks=1)[0].to_bytes(w, "big")
                    for k, i in enumerate(indices))


def err(nat):
    return nat.lib().hb_last_error(nat.context().h).decode()


# ------------------------------------------------------------------ 1: the golden cases, reversed
def test_golden_cases_in_reversed_order(nat, golden_encode):
    """Every golden case (prime, keys, data and tags from the unmodified
    reference), its blocks sent last first.  Only the last LISTED block of a
    call may be short, and a file's last block always is, so it goes first in
    a call of its own and the whole blocks follow, reversed, in a second."""
    n = 0
    for c in golden_encode["cases"]:
        p, S = int(c["prime"], 16), c["sectors"]
        fk, ak, data = bytes.fromhex(c["f_key"]), bytes.fromhex(c["alpha_key"]), bytes.fromhex(c["data"])
        w = nat.width_of(p)
        C = (p.bit_length() // 8) * S
        want = [int(t, 16).to_bytes(w, "big") for t in c["tags"]]
        nb = len(want)
        assert nb == len(data) // C + 1
        rc, last, _ = blocks_one(nat, p, S, fk, ak, [nb - 1], data[(nb - 1) * C:])
        assert rc == 0, err(nat)
        assert last == want[nb - 1], c["name"]
        order = list(range(nb - 2, -1, -1))
        rc, got, _ = blocks_one(nat, p, S, fk, ak, order, b"".join(data[i * C:(i + 1) * C] for i in order))
        assert rc == 0, err(nat)
        assert got == b"".join(want[i] for i in order), c["name"]
        n += 1
    assert n == 176


# ------------------------------------------------------------------ 2: indices
S1, SS1, C1 = 16, 32, 512
EDGES = [2 ** 64 - 1, 0, 9, 2 ** 63, 10, 99999, 2 ** 32, 9, 2 ** 32 - 1, 10 ** 19, 99999999999]   # unsorted, 9 twice


def test_indices_up_to_2_64_in_one_call(nat, oracle):
    fk, ak = _keys(2, 1)[0]
    data = _bytes(2, len(EDGES) * C1 - 100)
    rc, got, tries = blocks_one(nat, P256, S1, fk, ak, EDGES, data)
    assert rc == 0, err(nat)
    assert got == ref_tags(oracle, P256, S1, fk, ak, EDGES, data)
    w = nat.width_of(P256)
    assert got[1 * w:2 * w] != got[3 * w:4 * w]                 # 0 and 2^63 ...
    assert got[6 * w:7 * w] != got[1 * w:2 * w]                 # ... and 2^32 are not index 0
    total = 0
    for k, i in enumerate(EDGES):
        one, t = single_block(nat, P256, S1, fk, ak, i, data[k * C1:(k + 1) * C1])
        assert got[k * w:(k + 1) * w] == one, i
        total += t
    assert tries == total                                       # the sum of the single calls' tries


# ------------------------------------------------------------------ 3: list sizes, against the whole file
@pytest.fixture(scope="module")
def file200(nat):
    """A 200-block file under one key pair and hb_encode's tags of it."""
    fk, ak = _keys(3, 1)[0]
    data = _bytes(3, 199 * C1 + 77)
    return fk, ak, data, whole_file(nat, P256, S1, fk, ak, data)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 3 * 64 + 1])
def test_list_sizes(nat, oracle, file200, count):
    fk, ak, data, whole = file200
    w = nat.width_of(P256)
    idx = random.Random(count).sample(range(199), count - 1) + [199]      # unsorted, the short last block last
    packed = b"".join(data[i * C1:(i + 1) * C1] for i in idx)
    rc, got, tries = blocks_one(nat, P256, S1, fk, ak, idx, packed)
    assert rc == 0, err(nat)
    assert got == b"".join(whole[i * w:(i + 1) * w] for i in idx)          # hb_encode of the whole file at those indices
    assert got == ref_tags(oracle, P256, S1, fk, ak, idx, packed)
    assert tries >= count


def test_forced_split_into_three_groups(nat, file200, monkeypatch):
    fk, ak, data, whole = file200
    w = nat.width_of(P256)
    idx = list(range(150, 100, -1))                             # 50 blocks under a cap of 20: 20 + 20 + 10
    packed = b"".join(data[i * C1:(i + 1) * C1] for i in idx)
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", "20")
    try:
        rc, got, _ = blocks_one(nat, P256, S1, fk, ak, idx, packed)
        launches = nat.context().last_kernel_ms()[1]
        # two files of 15: (15, 5) and (10): a list that starts in one group and ends in the next
        rc2, got2, _ = blocks_many(nat, P256, S1, [(fk, ak, idx[:15], packed[:15 * C1]), (ak, fk, idx[15:30], packed[15 * C1:30 * C1])])
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0 and rc2 == 0, err(nat)
    assert got == b"".join(whole[i * w:(i + 1) * w] for i in idx)
    assert launches == 6                                        # a PRF and a MAC launch per group
    assert got2[0] == got[:15 * w]
    rc, want, _ = blocks_one(nat, P256, S1, ak, fk, idx[15:30], packed[15 * C1:30 * C1])
    assert rc == 0 and got2[1] == want


# ------------------------------------------------------------------ 4: the last listed block's length
@pytest.mark.parametrize("last", [0, 1, SS1 - 1, SS1, SS1 + 1, C1 - 1, C1])
def test_last_block_lengths(nat, oracle, last):
    fk, ak = _keys(4, 1)[0]
    idx = [7, 2 ** 40, 3]
    data = _bytes(40 + last, 2 * C1 + last)
    rc, got, _ = blocks_one(nat, P256, S1, fk, ak, idx, data)
    assert rc == 0, err(nat)
    assert got == ref_tags(oracle, P256, S1, fk, ak, idx, data)
    if last == 0:                                               # an empty block: tag = F(index)
        w = nat.width_of(P256)
        assert int.from_bytes(got[2 * w:], "big") == oracle.prf_eval(fk, P256, 3)


# ------------------------------------------------------------------ 5: limb counts, key lengths, sector counts
@pytest.mark.parametrize("bits,S,klen", [
    (61, 3, 16),       # a prime of two 32-bit limbs, 7-byte sectors, AES-128
    (256, 1, 24),      # S = 1: a lane per block, AES-192
    (256, 10, 32),
    (256, 300, 32),    # above the sector-parallel MAC's width
    (384, 5, 32),      # 48-byte sectors: no 16-byte loads
    (512, 16, 16),
    (1024, 10, 32),    # PySwizzle's defaults
    (2048, 4, 24),     # 64 limbs
])
def test_batch_shapes(nat, oracle, bits, S, klen):
    p = P256 if bits == 256 else _prime(bits, 11 * bits + S)
    ss = p.bit_length() // 8
    C = ss * S
    keys = _keys(bits + S, 3, klen)
    files = []
    for f, (fk, ak) in enumerate(keys):
        count = (1, 17, 70)[f]
        idx = [(2 ** 64 - 1 - k * 10 ** 17) if k % 3 == 0 else 5 * k + f for k in range(count)]
        files.append((fk, ak, idx, _bytes(1000 * f + bits, (count - 1) * C + (0, min(ss + 1, C), C - 1)[f])))
    rc, got, tries = blocks_many(nat, p, S, files)
    assert rc == 0, err(nat)
    for f, (fk, ak, idx, data) in enumerate(files):
        assert got[f] == ref_tags(oracle, p, S, fk, ak, idx, data), f
    assert tries >= 88


# ------------------------------------------------------------------ 6: batches of files
@pytest.mark.parametrize("nfiles", [3, 70])
def test_files_with_their_own_keys(nat, oracle, nfiles):
    keys = _keys(60 + nfiles, nfiles)
    rng = random.Random(nfiles)
    files = []
    for f, (fk, ak) in enumerate(keys):
        count = 0 if f == 1 else rng.randrange(1, 6)            # an empty list between two others
        idx = [rng.randrange(0, 1000) for _ in range(count)]
        tail = rng.choice([0, 5, C1]) if count else 0
        files.append((fk, ak, idx, _bytes(7 * f, max(count - 1, 0) * C1 + tail)))
    rc, got, tries = blocks_many(nat, P256, S1, files)
    assert rc == 0, err(nat)
    w = nat.width_of(P256)
    total = 0
    for f, (fk, ak, idx, data) in enumerate(files):
        assert got[f] == ref_tags(oracle, P256, S1, fk, ak, idx, data), f
        for k, i in enumerate(idx):
            one, t = single_block(nat, P256, S1, fk, ak, i, data[k * C1:(k + 1) * C1])
            assert got[f][k * w:(k + 1) * w] == one
            total += t
    assert got[1] == b""
    assert tries == total


def test_empty_calls(nat):
    rc, got, tries = blocks_many(nat, P256, S1, [])
    assert rc == 0 and tries == 0
    fk, ak = _keys(1, 1)[0]
    rc, got, tries = blocks_many(nat, P256, S1, [(fk, ak, [], b""), (fk, ak, [], b"")])
    assert rc == 0 and got == [b"", b""] and tries == 0


# ------------------------------------------------------------------ 7: device-resident, odd addresses
def test_device_resident_odd_addresses(nat, oracle):
    keys = _keys(70, 4)
    files = [(fk, ak, [2 ** 64 - 1 - f, f, 3], _bytes(70 + f, 2 * C1 + (0, 1, 33, C1)[f])) for f, (fk, ak) in enumerate(keys)]
    w = nat.width_of(P256)
    doffs, toffs, d, t = [], [], 1, 3
    for _, _, idx, data in files:
        doffs.append(d)
        toffs.append(t)
        d = (d + len(data) + 2) | 1
        t = (t + len(idx) * w + 2) | 1
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    try:
        for (_, _, _, data), o in zip(files, doffs):
            dbuf.upload(data, o)
        rc, _, _ = blocks_many(nat, P256, S1, files, flags=3, data_ptrs=[dbuf.p + o for o in doffs],
                               tag_ptrs=[tbuf.p + o for o in toffs])
        assert rc == 0, err(nat)
        raw = tbuf.download()
        # host data, device tags; device data, host tags
        rc, _, _ = blocks_many(nat, P256, S1, files[:2], flags=2, tag_ptrs=[tbuf.p + o for o in toffs[:2]])
        assert rc == 0, err(nat)
        raw2 = tbuf.download()
        rc, got3, _ = blocks_many(nat, P256, S1, files, flags=1, data_ptrs=[dbuf.p + o for o in doffs])
        assert rc == 0, err(nat)
    finally:
        dbuf.free()
        tbuf.free()
    for f, (fk, ak, idx, data) in enumerate(files):
        want = ref_tags(oracle, P256, S1, fk, ak, idx, data)
        assert raw[toffs[f]:toffs[f] + len(want)] == want, f
        assert got3[f] == want, f
        if f < 2:
            assert raw2[toffs[f]:toffs[f] + len(want)] == want, f


# ------------------------------------------------------------------ 8: errors, and the context afterwards
def test_errors_write_no_tag_and_leave_the_context_clean(nat, oracle):
    pys = importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")
    keys = _keys(80, 3)
    files = [(fk, ak, [5, 6], _bytes(80 + f, C1 + 9)) for f, (fk, ak) in enumerate(keys)]
    for flag in ("HB_PRF_CXX", "HB_ASYNC", "HB_ENCODE_SINGLE_PASS", "HB_HOST_REGISTER"):
        rc, got, _ = blocks_many(nat, P256, S1, files, flags=getattr(nat, flag), fill=0xA5)
        assert rc == nat.HB_EUNSUPPORTED, flag
        assert all(set(g) == {0xA5} for g in got)
    HB_EINVAL = -1

    def bad(spoil, msg):
        ctx = nat.context()
        w = nat.width_of(P256)
        descs = (nat.BlocksDesc * 3)()
        keep = []
        for i, (fk, ak, idx, data) in enumerate(files):
            ia, da, out = np.array(idx, dtype=np.uint64), np.frombuffer(data, dtype=np.uint8), np.full(2 * w, 0xA5, dtype=np.uint8)
            keep.append((ia, da, out))
            d = descs[i]
            d.f_key, d.alpha_key, d.indices, d.nblocks = fk, ak, ia.ctypes.data, 2
            d.data, d.len, d.tags = da.ctypes.data, len(data), out.ctypes.data
        spoil(descs[1])
        pb = nat.be(P256)
        with ctx.lock:
            rc = nat.lib().hb_encode_blocks_many(ctx.h, pb, len(pb), S1, 32, descs, 3, 0, None)
        assert rc == HB_EINVAL, msg
        assert err(nat) == msg
        assert all(set(out.tolist()) == {0xA5} for _, _, out in keep), msg

    bad(lambda d: setattr(d, "len", 2 * C1 + 1), "file 1: len is outside [(nblocks - 1) * C, nblocks * C]")
    bad(lambda d: setattr(d, "len", C1 - 1), "file 1: len is outside [(nblocks - 1) * C, nblocks * C]")
    bad(lambda d: setattr(d, "f_key", None), "file 1: a key is NULL")
    bad(lambda d: setattr(d, "indices", None), "file 1: indices is NULL")
    bad(lambda d: setattr(d, "tags", None), "file 1: tags buffer is NULL")
    bad(lambda d: setattr(d, "data", None), "file 1: data buffer is NULL")
    # afterwards: the call itself, a plain encode, a prove and a verify agree with the oracle
    rc, got, _ = blocks_many(nat, P256, S1, files)
    assert rc == 0, err(nat)
    for f, (fk, ak, idx, data) in enumerate(files):
        assert got[f] == ref_tags(oracle, P256, S1, fk, ak, idx, data)
    data = _bytes(81, 9 * C1 + 5)
    beat = pys.PySwizzle(S1, b"k" * 32, P256)
    tag, state = beat.encode(io.BytesIO(data))
    chal = pys.Challenge(40, P256, b"c" * 32)
    proof = beat.get_public().prove(io.BytesIO(data), chal, tag)
    mu, sg = oracle.prove(P256, S1, b"c" * 32, 40, P256, tag.sigma, data)
    assert proof.mu == mu and proof.sigma == sg
    assert beat.verify(proof, chal, state)
    assert tag.sigma == oracle.encode(P256, S1, state.f_key, state.alpha_key, data)
