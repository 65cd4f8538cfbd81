"""GPU parity of the cxx listed-block encode (hb_cxx_encode_blocks,
hb_cxx_encode_blocks_many): tags[k] of a file are the bytes hb_encode writes
with HB_PRF_CXX for block_base = indices[k], the k-th packed block and
nblocks = 1.

cxx parity is unpinned (no Crypto++ here, no recorded outputs), so there are
two references, and every check uses both where the indices lie inside a file:
oracle.cxx_encode(..., block_base=i, nblocks=1) -- the body of
cxx/shacham_waters_private.cxx:674-694 for one chunk_id -- and the existing
hb_encode(HB_PRF_CXX) of the whole file read at the listed indices (elsewhere:
of the single block).

* list sizes around the wave-job (HB_CB_JOB = 64) out of a 200-block file,
* unsorted and repeated indices with 0 and 2^32 - 1; 2^32 is refused,
* every length of the last listed block; a list of one empty block,
* limb counts, key lengths, S = 1 / 10 / above the sector-parallel MAC,
* a forced split into three groups whose last block is empty,
* batches of files with their own keys, an empty list among them, tries,
* device-resident data and tags at odd addresses,
* the order of the checks, unsupported flags, a 257-bit prime and bad
  descriptors, and the context afterwards."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_blocks import _bytes, _keys, _prime, blocks_one, err, ref_tags
from test_gpu_cxx import P1024
from test_gpu_cxx_many import encode_many, oracle_raw
from test_gpu_parity import P256, DevBuf

pytestmark = pytest.mark.gpu

HB_EINVAL = -1
S, SS, C, W = 10, 128, 1280, 128          # the cxx Swizzle's defaults: a 1024-bit prime, 10 sectors


@pytest.fixture(scope="module")
def nat():
    from heartbeat_amd import _native
    _native.context()
    return _native


def cblocks_many(nat, p, sectors, files, flags=0, fill=None, data_ptrs=None, tag_ptrs=None, klen=None):
    """hb_cxx_encode_blocks_many over files = [(f_key, alpha_key, indices,
    packed bytes)]: (rc, [tag bytes per file] for host tags, tries)."""
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
        rc = nat.lib().hb_cxx_encode_blocks_many(ctx.h, pb, len(pb), sectors, klen, descs, n, flags, ctypes.byref(tries))
    return rc, [o.tobytes() for o in outs], tries.value


def cblocks_one(nat, p, sectors, fk, ak, indices, data, flags=0):
    """hb_cxx_encode_blocks: (rc, tag bytes, tries)."""
    ctx = nat.context()
    w = nat.width_of(p)
    idx = np.array(indices, dtype=np.uint64)
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(len(idx) * w, dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        rc = nat.lib().hb_cxx_encode_blocks(ctx.h, pb, len(pb), sectors, fk, ak, len(fk),
                                            idx.ctypes.data if len(idx) else None, len(idx),
                                            a.ctypes.data if len(a) else None, len(data),
                                            out.ctypes.data if len(idx) else None, flags, ctypes.byref(tries))
    return rc, out.tobytes(), tries.value


def single_block(nat, p, sectors, fk, ak, index, data):
    """hb_encode(HB_PRF_CXX) of one block at block_base = index: (tag bytes, tries)."""
    ctx = nat.context()
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(nat.width_of(p), dtype=np.uint8)
    pb = nat.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), sectors, fk, ak, len(fk), index, a.ctypes.data if len(a) else None,
                                      len(data), 1, out.ctypes.data, nat.HB_PRF_CXX, ctypes.byref(tries)))
    return out.tobytes(), tries.value


def whole_file(nat, p, sectors, fk, ak, data):
    """hb_encode(HB_PRF_CXX) of a whole file: its tag bytes."""
    ctx = nat.context()
    nb = len(data) // ((p.bit_length() // 8) * sectors) + 1
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(nb * nat.width_of(p), dtype=np.uint8)
    pb = nat.be(p)
    with ctx.lock:
        ctx.check(nat.lib().hb_encode(ctx.h, pb, len(pb), sectors, fk, ak, len(fk), 0, a.ctypes.data if len(a) else None,
                                      len(data), nb, out.ctypes.data, nat.HB_PRF_CXX, None))
    return out.tobytes()


def cref_tags(oracle, p, sectors, fk, ak, indices, data):
    """The first reference: one oracle.cxx_encode(block_base=i, nblocks=1) per listed block."""
    w = (p.bit_length() + 7) // 8
    c = (p.bit_length() // 8) * sectors
    return b"".join(oracle.cxx_encode(p, sectors, fk, ak, data[k * c:(k + 1) * c], block_base=int(i), nblocks=1)[0]
                    .to_bytes(w, "big") for k, i in enumerate(indices))


def singles(nat, p, sectors, fk, ak, indices, data):
    """The second reference outside a file: (tag bytes, tries) of one hb_encode(HB_PRF_CXX) per listed block."""
    c = (p.bit_length() // 8) * sectors
    got = [single_block(nat, p, sectors, fk, ak, int(i), data[k * c:(k + 1) * c]) for k, i in enumerate(indices)]
    return b"".join(t for t, _ in got), sum(n for _, n in got)


# ------------------------------------------------------------------ 1: list sizes, against the whole file
@pytest.fixture(scope="module")
def file200(nat):
    """A 200-block file under one key pair and hb_encode(HB_PRF_CXX)'s tags of it."""
    fk, ak = _keys(3, 1)[0]
    data = _bytes(3, 199 * C + 77)
    return fk, ak, data, whole_file(nat, P1024, S, fk, ak, data)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_list_sizes(nat, oracle, file200, count):
    fk, ak, data, whole = file200
    idx = random.Random(count).sample(range(199), count - 1) + [199]      # unsorted, the short last block last
    packed = b"".join(data[i * C:(i + 1) * C] for i in idx)
    rc, got, tries = cblocks_one(nat, P1024, S, fk, ak, idx, packed)
    assert rc == 0, err(nat)
    assert got == b"".join(whole[i * W:(i + 1) * W] for i in idx)          # the whole file's tags at those indices
    assert got == cref_tags(oracle, P1024, S, fk, ak, idx, packed)
    assert tries >= count


# ------------------------------------------------------------------ 2: indices
EDGES = [2 ** 32 - 1, 0, 9, 2 ** 31, 10, 99999, 9, 2 ** 32 - 2, 0]       # unsorted, 9 and 0 twice


def test_unsorted_repeated_indices_and_the_u32_bound(nat, oracle):
    fk, ak = _keys(2, 1)[0]
    data = _bytes(2, len(EDGES) * C - 100)
    rc, got, tries = cblocks_one(nat, P1024, S, fk, ak, EDGES, data)
    assert rc == 0, err(nat)
    assert got == cref_tags(oracle, P1024, S, fk, ak, EDGES, data)
    one, total = singles(nat, P1024, S, fk, ak, EDGES, data)
    assert got == one
    assert tries == total                                       # the sum of the single calls' tries
    assert got[0:W] != got[W:2 * W]                             # 2^32 - 1 is not index 0 ...
    # ... and 2^32 is refused, not wrapped to it: in the second file of a call, naming it; no buffer is written
    for wide in (2 ** 32, 2 ** 64 - 1):
        files = [(fk, ak, [1, 2], data[:2 * C]), (ak, fk, [0, wide, 3], data[:3 * C])]
        rc, out, tries = cblocks_many(nat, P1024, S, files, fill=0xA5)
        assert rc == nat.HB_EUNSUPPORTED and tries == 0
        assert err(nat) == "file 1: index %d (listed block 1) does not fit the cxx prf's unsigned int" % wide
        assert all(set(o) == {0xA5} for o in out)
    rc, out, _ = cblocks_many(nat, P1024, S, [(fk, ak, [1, 2], data[:2 * C])])
    assert rc == 0 and out[0] == cref_tags(oracle, P1024, S, fk, ak, [1, 2], data[:2 * C])


# ------------------------------------------------------------------ 3: the last listed block's length
@pytest.mark.parametrize("last", [0, 1, SS - 1, SS, SS + 1, C - 1, C])
def test_last_block_lengths(nat, oracle, last):
    fk, ak = _keys(4, 1)[0]
    idx = [7, 2 ** 31, 3]
    data = _bytes(40 + last, 2 * C + last)
    rc, got, tries = cblocks_one(nat, P1024, S, fk, ak, idx, data)
    assert rc == 0, err(nat)
    assert got == cref_tags(oracle, P1024, S, fk, ak, idx, data)
    one, total = singles(nat, P1024, S, fk, ak, idx, data)
    assert got == one and tries == total
    if last == 0:                                               # an empty block: the tag is F(index) as the prf returned it
        assert int.from_bytes(got[2 * W:], "big") == oracle.cxx_prf_eval(fk, P1024, 3)[0]


def test_a_list_of_one_empty_block_is_the_unreduced_f(nat, oracle):
    """No block reads a sector: the group has no MAC launch, and the tag is F
    as the prf returned it, without `%= p`, equal to the single call's."""
    fk, ak = _keys(5, 1)[0]
    for index in (0, 5, 2 ** 32 - 1):
        rc, got, tries = cblocks_one(nat, P1024, S, fk, ak, [index], b"")
        assert rc == 0, err(nat)
        one, t = single_block(nat, P1024, S, fk, ak, index, b"")
        assert got == one and tries == t
        f, ft = oracle.cxx_prf_eval(fk, P1024, index)
        assert int.from_bytes(got, "big") == f and tries == ft
    assert nat.context().last_kernel_ms()[1] == 2               # the PRF launch and the Montgomery pass, no MAC


# ------------------------------------------------------------------ 4: limb counts, key lengths, sector counts
@pytest.mark.parametrize("bits,sectors,klen", [
    (256, 16, 16),
    (256, 1, 24),      # S = 1: one lane per block in the MAC
    (384, 3, 32),      # tag width 48 bytes: a multiple of 16 below 4 NL
    (512, 10, 32),
    (1024, 10, 32),    # the cxx Swizzle's defaults
    (2048, 3, 16),     # 64 limbs
    (256, 300, 32),    # above the sector-parallel MAC's width
])
def test_batch_shapes(nat, oracle, bits, sectors, klen):
    p = P256 if bits == 256 else P1024 if bits == 1024 else _prime(bits, 7 * bits + sectors)
    ss = p.bit_length() // 8
    c = ss * sectors
    keys = _keys(bits + sectors, 3, klen)
    files = []
    for f, (fk, ak) in enumerate(keys):
        count = (1, 17, 70)[f]
        idx = [(2 ** 32 - 1 - k * 10 ** 7) if k % 3 == 0 else 5 * k + f for k in range(count)]
        files.append((fk, ak, idx, _bytes(1000 * f + bits, (count - 1) * c + (0, min(ss + 1, c), c - 1)[f])))
    rc, got, tries = cblocks_many(nat, p, sectors, files)
    assert rc == 0, err(nat)
    total = 0
    for f, (fk, ak, idx, data) in enumerate(files):
        assert got[f] == cref_tags(oracle, p, sectors, fk, ak, idx, data), f
        if f < 2:                                               # the second reference on the two short lists
            one, t = singles(nat, p, sectors, fk, ak, idx, data)
            assert got[f] == one, f
            total += t
    assert tries >= total + 70


# ------------------------------------------------------------------ 5: a forced split
def test_forced_split_into_three_groups_with_an_empty_last_block(nat, oracle, file200, monkeypatch):
    fk, ak, data, whole = file200
    idx = list(range(150, 101, -1)) + [199]                     # 50 blocks under a cap of 20: 20 + 20 + 10
    packed = b"".join(data[i * C:(i + 1) * C] for i in idx[:49])          # the last listed block is empty
    rc, want, want_tries = cblocks_one(nat, P1024, S, fk, ak, idx, packed)
    assert rc == 0, err(nat)
    assert nat.context().last_kernel_ms()[1] == 3
    monkeypatch.setenv("HB_TEST_BATCH_BLOCKS", "20")
    try:
        rc, got, tries = cblocks_one(nat, P1024, S, fk, ak, idx, packed)
        launches = nat.context().last_kernel_ms()[1]
    finally:
        monkeypatch.delenv("HB_TEST_BATCH_BLOCKS", raising=False)
    assert rc == 0, err(nat)
    assert got == want and tries == want_tries                  # equal to the unsplit call
    assert launches == 9                                        # PRF, Montgomery and MAC per group
    assert got[:49 * W] == b"".join(whole[i * W:(i + 1) * W] for i in idx[:49])
    assert int.from_bytes(got[49 * W:], "big") == oracle.cxx_prf_eval(fk, P1024, 199)[0]
    assert got == cref_tags(oracle, P1024, S, fk, ak, idx, packed)


# ------------------------------------------------------------------ 6: batches of files
@pytest.mark.parametrize("nfiles", [1, 2, 33])
def test_files_with_their_own_keys(nat, oracle, nfiles):
    keys = _keys(60 + nfiles, nfiles)
    rng = random.Random(nfiles)
    files = []
    for f, (fk, ak) in enumerate(keys):
        count = 0 if f == 1 else rng.randrange(1, 6)            # an empty list among the others
        idx = [rng.randrange(0, 1000) for _ in range(count)]
        tail = rng.choice([0, 5, C]) if count else 0
        files.append((fk, ak, idx, _bytes(7 * f, max(count - 1, 0) * C + tail)))
    rc, got, tries = cblocks_many(nat, P1024, S, files)
    assert rc == 0, err(nat)
    total = 0
    for f, (fk, ak, idx, data) in enumerate(files):
        assert got[f] == cref_tags(oracle, P1024, S, fk, ak, idx, data), f
        one, t = singles(nat, P1024, S, fk, ak, idx, data)
        assert got[f] == one, f
        total += t
    if nfiles > 1:
        assert got[1] == b""
    assert tries == total


def test_empty_calls(nat):
    rc, got, tries = cblocks_many(nat, P1024, S, [])
    assert rc == 0 and tries == 0
    fk, ak = _keys(1, 1)[0]
    rc, got, tries = cblocks_many(nat, P1024, S, [(fk, ak, [], b""), (fk, ak, [], b"")])
    assert rc == 0 and got == [b"", b""] and tries == 0


# ------------------------------------------------------------------ 7: device-resident, odd addresses
def test_device_resident_odd_addresses(nat, oracle):
    keys = _keys(70, 4)
    files = [(fk, ak, [2 ** 32 - 1 - f, f, 3], _bytes(70 + f, 2 * C + (0, 1, 33, C)[f])) for f, (fk, ak) in enumerate(keys)]
    doffs, toffs, d, t = [], [], 1, 3
    for _, _, idx, data in files:
        doffs.append(d)
        toffs.append(t)
        d = (d + len(data) + 2) | 1
        t = (t + len(idx) * W + 2) | 1
    dbuf, tbuf = DevBuf(nat, d + 16), DevBuf(nat, t + 16)
    try:
        for (_, _, _, data), o in zip(files, doffs):
            dbuf.upload(data, o)
        rc, _, _ = cblocks_many(nat, P1024, S, files, flags=3, data_ptrs=[dbuf.p + o for o in doffs],
                                tag_ptrs=[tbuf.p + o for o in toffs])
        assert rc == 0, err(nat)
        raw = tbuf.download()
        # host data, device tags; device data, host tags
        rc, _, _ = cblocks_many(nat, P1024, S, files[:2], flags=2, tag_ptrs=[tbuf.p + o for o in toffs[:2]])
        assert rc == 0, err(nat)
        raw2 = tbuf.download()
        rc, got3, _ = cblocks_many(nat, P1024, S, files, flags=1, data_ptrs=[dbuf.p + o for o in doffs])
        assert rc == 0, err(nat)
    finally:
        dbuf.free()
        tbuf.free()
    for f, (fk, ak, idx, data) in enumerate(files):
        want = cref_tags(oracle, P1024, S, fk, ak, idx, data)
        assert singles(nat, P1024, S, fk, ak, idx, data)[0] == want, f
        assert raw[toffs[f]:toffs[f] + len(want)] == want, f
        assert got3[f] == want, f
        if f < 2:
            assert raw2[toffs[f]:toffs[f] + len(want)] == want, f


# ------------------------------------------------------------------ 8: errors, their order, and the context afterwards
def test_errors_write_no_tag_and_leave_the_context_clean(nat, oracle):
    keys = _keys(80, 3)
    files = [(fk, ak, [5, 6], _bytes(80 + f, C + 9)) for f, (fk, ak) in enumerate(keys)]

    def valid():
        rc, got, _ = cblocks_many(nat, P1024, S, files)
        assert rc == 0, err(nat)
        for f, (fk, ak, idx, data) in enumerate(files):
            assert got[f] == cref_tags(oracle, P1024, S, fk, ak, idx, data)

    for flag in ("HB_PRF_CXX", "HB_ASYNC", "HB_ENCODE_SINGLE_PASS", "HB_HOST_REGISTER"):
        rc, got, _ = cblocks_many(nat, P1024, S, files, flags=getattr(nat, flag), fill=0xA5)
        assert rc == nat.HB_EUNSUPPORTED, flag
        assert err(nat) == "hb_cxx_encode_blocks_many takes HB_DATA_ON_DEVICE and HB_TAGS_ON_DEVICE only"
        assert all(set(g) == {0xA5} for g in got)
        valid()
    # a 257-bit prime: ByteCount 33, the code hb_encode(HB_PRF_CXX) returns for it
    p257 = _prime(257, 257)
    files257 = [(fk, ak, [5, 6], _bytes(90 + f, 32 * S + 9)) for f, (fk, ak) in enumerate(keys)]
    rc, got, _ = cblocks_many(nat, p257, S, files257, fill=0xA5)
    assert rc == nat.HB_EUNSUPPORTED and err(nat) == "cxx prf mode needs ByteCount(p) to be a multiple of 16"
    assert all(set(g) == {0xA5} for g in got)
    ctx = nat.context()
    a = np.frombuffer(files257[0][3], dtype=np.uint8)
    out = np.empty(33, dtype=np.uint8)
    pb = nat.be(p257)
    with ctx.lock:
        assert nat.lib().hb_encode(ctx.h, pb, len(pb), S, keys[0][0], keys[0][1], 32, 5, a.ctypes.data, 32 * S, 1,
                                   out.ctypes.data, nat.HB_PRF_CXX, None) == nat.HB_EUNSUPPORTED
    valid()

    def bad(spoil, msg, code=HB_EINVAL, p=P1024, flags=0):
        w = nat.width_of(p)
        descs = (nat.BlocksDesc * 3)()
        keep = []
        for i, (fk, ak, idx, data) in enumerate(files if p == P1024 else files257):
            ia, da, out = np.array(idx, dtype=np.uint64), np.frombuffer(data, dtype=np.uint8), np.full(2 * w, 0xA5, dtype=np.uint8)
            keep.append((ia, da, out))
            d = descs[i]
            d.f_key, d.alpha_key, d.indices, d.nblocks = fk, ak, ia.ctypes.data, 2
            d.data, d.len, d.tags = da.ctypes.data, len(data), out.ctypes.data
        spoil(descs, keep)
        pb = nat.be(p)
        with ctx.lock:
            rc = nat.lib().hb_cxx_encode_blocks_many(ctx.h, pb, len(pb), S, 32, descs, 3, flags, None)
        assert rc == code, msg
        assert err(nat) == msg
        assert all(set(out.tolist()) == {0xA5} for _, _, out in keep), msg
        valid()

    def wide(descs, keep, f=0):
        keep[f][0][1] = 2 ** 32

    bad(lambda d, k: setattr(d[1], "len", 2 * C + 1), "file 1: len is outside [(nblocks - 1) * C, nblocks * C]")
    bad(lambda d, k: setattr(d[1], "len", C - 1), "file 1: len is outside [(nblocks - 1) * C, nblocks * C]")
    bad(lambda d, k: setattr(d[1], "f_key", None), "file 1: a key is NULL")
    bad(lambda d, k: setattr(d[1], "indices", None), "file 1: indices is NULL")
    bad(lambda d, k: setattr(d[1], "tags", None), "file 1: tags buffer is NULL")
    bad(lambda d, k: setattr(d[1], "data", None), "file 1: data buffer is NULL")
    # the order: flags, descriptors (a later file's too), indices, the prime's ByteCount
    wide_msg = "file 0: index 4294967296 (listed block 1) does not fit the cxx prf's unsigned int"
    bad(wide, wide_msg, nat.HB_EUNSUPPORTED)
    bad(lambda d, k: (wide(d, k), setattr(d[2], "tags", None)), "file 2: tags buffer is NULL")
    bad(lambda d, k: (wide(d, k), setattr(d[2], "tags", None)),
        "hb_cxx_encode_blocks_many takes HB_DATA_ON_DEVICE and HB_TAGS_ON_DEVICE only", nat.HB_EUNSUPPORTED, flags=nat.HB_ASYNC)
    bad(wide, wide_msg, nat.HB_EUNSUPPORTED, p=p257)
    bad(lambda d, k: setattr(d[2], "data", None), "file 2: data buffer is NULL", p=p257)
    # afterwards the context still does a cxx encode_many and a PySwizzle encode_blocks
    datas = [_bytes(95 + f, 3 * C + f) for f in range(3)]
    rc, got, _ = encode_many(nat, P1024, S, keys, datas)
    assert rc == 0, err(nat)
    for f in range(3):
        assert got[f] == oracle_raw(oracle, P1024, S, keys[f][0], keys[f][1], datas[f], W)
    rc, got, _ = blocks_one(nat, P256, 16, keys[0][0], keys[0][1], [2 ** 40, 1], _bytes(99, 512 + 7))
    assert rc == 0, err(nat)
    assert got == ref_tags(oracle, P256, 16, keys[0][0], keys[0][1], [2 ** 40, 1], _bytes(99, 512 + 7))
