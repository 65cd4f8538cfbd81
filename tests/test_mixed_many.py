"""CPU tests of the mixed-owner batches' Python layer (heartbeat_amd._many:
prove_files_mixed, verify_rhs_mixed; PySwizzle.prove_mixed / verify_mixed) over
a small stand-in for libhbswizzle.so whose hb_prove_mixed / hb_verify_rhs_mixed
read each descriptor's raw words and answer with the CPU oracle -- no GPU.

Three beats -- a 256-bit prime with S = 16, a 1024-bit one with S = 10, a
61-bit one with S = 3 -- interleaved in one call.

Reference: a storage node's loop of b.prove(...) over the challenges of many
owners (PySwizzle.py:333-370, one prime per PySwizzle instance, :250-251) and
an auditor's loop of b.verify(...) (:372-395)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError
from test_prove_many import ProveLib, _prove
from test_verify_many import _rhs

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
# odd numbers of the right bit lengths: the oracle and the stand-in need no primality
P1024 = (1 << 1023) | int.from_bytes(bytes(range(1, 128)), "big") | 1
P61 = (1 << 60) | 0x123456789abcdf
BEATS = [(P256, 16), (P1024, 10), (P61, 3)]
KEYS = [b"A" * 32, b"B" * 32, b"C" * 32]


class MixedLib(ProveLib):
    """ProveLib's context and single prove, the single verify, and the two
    mixed calls reading each descriptor's fourteen raw words."""

    def __init__(self):
        ProveLib.__init__(self)
        self.mixed = []          # per call: [(p, S, key_len, ...)] as the descriptors carried them
        self.vsingle = 0

    def hb_prove_mixed(self, h, descs, n, flags):
        seen = []
        for i in range(n):
            # p_be, p_len, sectors, key_len, then hb_prove_desc's ten words
            x = (ctypes.c_uint64 * 14).from_address(ctypes.addressof(descs[i]))
            p = int.from_bytes(ctypes.string_at(x[0], x[1]), "big")
            S, klen = int(x[2]), int(x[3])
            w = (p.bit_length() + 7) // 8
            seen.append((p, S, klen))
            r = _prove(p, S, ctypes.string_at(x[4], klen), x[5], int.from_bytes(ctypes.string_at(x[6], x[7]), "big"),
                       x[8], x[9], x[10], x[11])
            ctypes.memmove(x[12], r[:S * w], S * w)
            ctypes.memmove(x[13], r[S * w:], w)
        self.mixed.append(("prove", int(flags), seen))
        return 0

    def hb_verify_rhs(self, h, pb, plen, sectors, fk, ak, klen, nstate, ck, cklen, chunks, vmax, vlen, mub, rhs):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.vsingle += 1
        mu = [int.from_bytes(mub[j * w:(j + 1) * w], "big") for j in range(sectors)]
        r = _rhs(p, sectors, fk[:klen], ak[:klen], nstate, ck[:cklen], chunks, int.from_bytes(vmax[:vlen], "big"), mu)
        ctypes.memmove(rhs, r.to_bytes(w, "big"), w)
        return 0

    def hb_verify_rhs_mixed(self, h, descs, n, flags):
        seen = []
        for i in range(n):
            # p_be, p_len, sectors, key_len, chal_key_len, then hb_verify_desc's nine words
            x = (ctypes.c_uint64 * 14).from_address(ctypes.addressof(descs[i]))
            p = int.from_bytes(ctypes.string_at(x[0], x[1]), "big")
            S, klen, cklen = int(x[2]), int(x[3]), int(x[4])
            w = (p.bit_length() + 7) // 8
            seen.append((p, S, klen, cklen))
            fk, ak, ck = ctypes.string_at(x[5], klen), ctypes.string_at(x[6], klen), ctypes.string_at(x[7], cklen)
            vmax = int.from_bytes(ctypes.string_at(x[10], x[11]), "big")
            mub = ctypes.string_at(x[12], S * w)
            mu = [int.from_bytes(mub[j * w:(j + 1) * w], "big") for j in range(S)]
            r = _rhs(p, S, fk, ak, x[8], ck, x[9], vmax, mu)
            ctypes.memmove(x[13], r.to_bytes(w, "big"), w)
        self.mixed.append(("verify", int(flags), seen))
        return 0


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = MixedLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])

    def xor_cfb8(key, iv, data, encrypt):                      # a reversible stand-in for hb_aes_cfb8
        pad = (bytes(key) + bytes(iv)) * (len(data) // 16 + 1)
        return bytes(a ^ b for a, b in zip(bytes(data), pad))

    monkeypatch.setattr(_native, "aes_cfb8", xor_cfb8)
    return fake


_cache = {}


def _material(oracle, k, cklen):
    """Item k's beat index, file bytes, keys, tags and honest proof (computed once)."""
    if (k, cklen) not in _cache:
        b = k % 3
        p, S = BEATS[b]
        data = bytes((11 * k + i) & 0xff for i in range(150 + 61 * (k % 4)))
        fk, ak, ck = bytes([k + 1]) * 32, bytes([0x80 + k]) * 32, bytes([0x40 + k]) * cklen
        tags = oracle.encode(p, S, fk, ak, data)
        chunks = len(tags) + (k % 2)
        mu, sigma = oracle.prove(p, S, ck, chunks, p, tags, data)
        _cache[(k, cklen)] = (b, data, fk, ak, ck, list(tags), chunks, mu, sigma)
    return _cache[(k, cklen)]


def _beats(pys):
    return [pys.PySwizzle(S, key, p) for (p, S), key in zip(BEATS, KEYS)]


def _prove_items(pys, oracle, n, cklens=(32,)):
    """n (beat, file, chal, tag), beats interleaved."""
    beats = _beats(pys)
    out = []
    for k in range(n):
        b, data, fk, ak, ck, tags, chunks, mu, sigma = _material(oracle, k, cklens[k % len(cklens)])
        tag = pys.Tag()
        tag.sigma = list(tags)
        out.append((beats[b], io.BytesIO(data), pys.Challenge(chunks, BEATS[b][0], ck), tag))
    return out


def _verify_items(pys, oracle, n):
    """n honest (beat, proof, chal, state), beats interleaved, each state under its own beat's key."""
    beats = _beats(pys)
    out = []
    for k in range(n):
        b, data, fk, ak, ck, tags, chunks, mu, sigma = _material(oracle, k, 32)
        proof = pys.Proof()
        proof.mu, proof.sigma = list(mu), sigma
        state = pys.State(fk, ak, len(tags))
        state.encrypt(beats[b].key)
        out.append((beats[b], proof, pys.Challenge(chunks, BEATS[b][0], ck), state))
    return out


def _pairs(proofs):
    return [(x.mu, x.sigma) for x in proofs]


def test_prove_mixed_equals_loop_and_descriptors(lib, oracle, pys):
    items = _prove_items(pys, oracle, 7, cklens=(32, 16, 24, 32))
    want = [b.prove(f, c, t) for b, f, c, t in items]
    assert lib.single == 7 and lib.mixed == []
    for (b, f, chal, tag), x in zip(items, want):               # the stand-in is the oracle's prove
        assert (x.mu, x.sigma) == tuple(oracle.prove(b.prime, b.sectors, chal.key, chal.chunks, b.prime, tag.sigma,
                                                     f.getvalue()))
    got = pys.PySwizzle.prove_mixed(items)
    assert _pairs(got) == _pairs(want)
    assert all(isinstance(g, pys.Proof) for g in got)
    assert lib.single == 7                                      # no single call beside the one mixed call
    (kind, flags, seen), = lib.mixed
    assert (kind, flags) == ("prove", 0)
    # every descriptor carries its own item's prime, S and key length
    assert seen == [(int(b.prime), int(b.sectors), len(c.key)) for b, f, c, t in items]
    assert len({s[0] for s in seen}) == 3 and {s[2] for s in seen} == {16, 24, 32}
    assert _pairs(pys.PySwizzle.prove_mixed(iter(items))) == _pairs(want)   # any iterable
    assert pys.PySwizzle.prove_mixed([]) == []


def test_prove_mixed_file_positions_restored(lib, oracle, pys, tmp_path):
    items = _prove_items(pys, oracle, 4)
    path = tmp_path / "f.bin"
    path.write_bytes(items[2][1].getvalue())
    with open(str(path), "rb") as fh:
        items[2] = (items[2][0], fh, items[2][2], items[2][3])
        items[0][1].seek(7)
        fh.seek(3)
        got = pys.PySwizzle.prove_mixed(items)
        assert [items[0][1].tell(), fh.tell()] == [7, 3]
        assert len(lib.mixed) == 1
        assert _pairs(got) == _pairs([b.prove(f, c, t) for b, f, c, t in items])
        assert [items[0][1].tell(), fh.tell()] == [7, 3]


def test_prove_mixed_zero_chunks_and_error_order(lib, oracle, pys):
    items = _prove_items(pys, oracle, 5)
    items[1][2].chunks = 0
    items[1] = items[1][:3] + (pys.Tag(),)                      # zero chunks and an empty tag: a zero proof
    items[3][2].chunks = -1
    want = [b.prove(f, c, t) for b, f, c, t in items]
    assert _pairs(want)[1] == ([0] * BEATS[1][1], 0) and _pairs(want)[3] == ([0] * BEATS[0][1], 0)
    singles = lib.single
    got = pys.PySwizzle.prove_mixed(items)
    assert _pairs(got) == _pairs(want)
    (kind, flags, seen), = lib.mixed
    assert len(seen) == 3 and lib.single == singles             # the zero proofs have no descriptor
    items[2] = items[2][:3] + (pys.Tag(),)                      # an empty tag with chunks > 0
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.prove_mixed(items)
    with pytest.raises(HeartbeatError) as e1:
        [b.prove(f, c, t) for b, f, c, t in items]
    assert str(e.value) == str(e1.value) == "tag is empty"
    assert len(lib.mixed) == 1                                  # nothing was called for the failing batch
    bad = pys.PySwizzle(0, b"K" * 32, P256)
    singles = lib.single
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.prove_mixed(items[:1] + [(bad,) + items[0][1:]])
    assert "sectors must be positive" in str(e.value)
    assert len(lib.mixed) == 1 and lib.single == singles


def test_prove_mixed_sharded_challenges_go_through_prove(lib, oracle, pys, monkeypatch):
    from heartbeat_amd import multi
    monkeypatch.setattr(multi, "_devices", [0, 0])
    monkeypatch.setattr(multi, "MIN_SHARD_CHUNKS", 6)
    items = _prove_items(pys, oracle, 4)
    for (b, f, chal, tag), n in zip(items, (3, 5, 12, 4)):
        chal.chunks = n
    got = pys.PySwizzle.prove_mixed(items)
    assert [len(m[2]) for m in lib.mixed] == [3]                # 12 chunks: through prove()
    for (b, f, chal, tag), g in zip(items, got):
        assert (g.mu, g.sigma) == tuple(oracle.prove(b.prime, b.sectors, chal.key, chal.chunks, b.prime, tag.sigma,
                                                     f.getvalue()))


def test_verify_mixed_equals_loop(lib, oracle, pys):
    items = _verify_items(pys, oracle, 6)
    items[1][1].mu[2] ^= 1                                      # a tampered mu
    items[4][1].sigma += 1                                      # a tampered sigma
    want = [b.verify(pr, c, s) for b, pr, c, s in items]
    assert want == [True, False, True, True, False, True] and lib.vsingle == 6
    items = _verify_items(pys, oracle, 6)                       # fresh (encrypted) states
    items[1][1].mu[2] ^= 1
    items[4][1].sigma += 1
    assert pys.PySwizzle.verify_mixed(items) == want
    assert lib.vsingle == 6
    (kind, flags, seen), = lib.mixed
    assert (kind, flags) == ("verify", 0)
    assert seen == [(int(b.prime), int(b.sectors), 32, 32) for b, pr, c, s in items]
    assert pys.PySwizzle.verify_mixed([]) == []


def test_verify_mixed_error_order(lib, oracle, pys):
    """A tampered state signature at item 2 while item 4 has too few mu: the
    loop's first error, and nothing is called on the library."""
    items = _verify_items(pys, oracle, 6)
    items[2][3].hmac = bytes(32)
    del items[4][1].mu[-1]
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.verify_mixed(items)
    assert str(e.value) == "Signature invalid on state."
    items2 = _verify_items(pys, oracle, 6)
    items2[2][3].hmac = bytes(32)
    del items2[4][1].mu[-1]
    with pytest.raises(HeartbeatError) as e1:
        [b.verify(pr, c, s) for b, pr, c, s in items2]
    assert str(e1.value) == str(e.value)
    assert lib.mixed == []
    items = _verify_items(pys, oracle, 6)
    del items[4][1].mu[-1]                                      # alone: too few mu values, under ITS beat's S
    vs = lib.vsingle
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.verify_mixed(items)
    assert str(e.value) == "proof has fewer than %d mu values" % BEATS[1][1]
    items = _verify_items(pys, oracle, 3)
    items[1][3].decrypt(items[1][0].key)
    items[1][3].chunks = 0
    items[1][3].hmac = items[1][3].get_hmac(items[1][0].key)
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.verify_mixed(items)
    assert str(e.value) == "state has no chunks"
    # a state under another beat's key: the loop's signature error
    items = _verify_items(pys, oracle, 3)
    items[0] = (items[1][0],) + items[0][1:]
    with pytest.raises(HeartbeatError) as e:
        pys.PySwizzle.verify_mixed(items)
    assert str(e.value) == "Signature invalid on state."
    assert lib.mixed == [] and lib.vsingle == vs


def test_many_functions_values(lib, oracle, pys):
    from heartbeat_amd import _many
    b, data, fk, ak, ck, tags, chunks, mu, sigma = _material(oracle, 1, 32)
    p, S = BEATS[b]
    tag = pys.Tag()
    tag.sigma = list(tags)
    got = _many.prove_files_mixed([(p, S, ck, chunks, p, tag, io.BytesIO(data)), (P61, 3, b"k" * 16, -2, 77, tag, b"")])
    assert got[0] == (mu, sigma)
    assert got[1] == ([0] * 3, 0)                               # chunks <= 0: zero sums
    rhs = _many.verify_rhs_mixed([(p, S, fk, ak, len(tags), ck, chunks, p, mu + [99]),
                                  (P61, 3, b"f" * 16, b"a" * 16, 1, b"d" * 24, 0, 77, [5, 6, P61 + 8])])
    assert rhs[0] == sigma
    assert rhs[1] == _rhs(P61, 3, b"f" * 16, b"a" * 16, 1, b"d" * 24, 0, 1, [5, 6, 8])
    assert lib.mixed[1][2][1] == (P61, 3, 16, 24)
    n = len(lib.mixed)
    with pytest.raises(HeartbeatError):
        _many.prove_files_mixed([(p, S, ck, 3, p, pys.Tag(), b"")])
    with pytest.raises(HeartbeatError):
        _many.prove_files_mixed([(p, 0, ck, 3, p, tag, b"")])
    with pytest.raises(HeartbeatError):
        _many.verify_rhs_mixed([(p, S, fk, ak, 1, ck, 1, p, mu[:-1])])
    assert _many.prove_files_mixed([]) == [] and _many.verify_rhs_mixed([]) == []
    assert len(lib.mixed) == n


def test_descriptor_layouts():
    """hb_prove_mixed_desc / hb_verify_mixed_desc (hbswizzle.h): fourteen
    8-byte words each, the one-prime descriptor's words last."""
    from heartbeat_amd import _native
    D = _native.ProveMixedDesc
    names = ["p_be", "p_len", "sectors", "key_len"] + [f[0] for f in _native.ProveDesc._fields_]
    assert ctypes.sizeof(D) == 112 and [f[0] for f in D._fields_] == names
    assert [getattr(D, n).offset for n in names] == list(range(0, 112, 8))
    V = _native.VerifyMixedDesc
    names = ["p_be", "p_len", "sectors", "key_len", "chal_key_len"] + [f[0] for f in _native.VerifyDesc._fields_]
    assert ctypes.sizeof(V) == 112 and [f[0] for f in V._fields_] == names
    assert [getattr(V, n).offset for n in names] == list(range(0, 112, 8))
    sig = {name: args for name, _, args in _native.SIGNATURES}
    assert sig["hb_prove_mixed"][1] == ctypes.POINTER(D) and len(sig["hb_prove_mixed"]) == 4
    assert sig["hb_verify_rhs_mixed"][1] == ctypes.POINTER(V) and len(sig["hb_verify_rhs_mixed"]) == 4
