"""CPU tests of the cxx mixed-owner batches' Python layer (heartbeat_amd.Swizzle:
prove_files_mixed, verify_rhs_mixed, Swizzle.prove_mixed / verify_mixed =
heartbeat.Heartbeat's; heartbeat_amd._many with the native name and the
exact_mu policy) over a small stand-in for libhbswizzle.so whose
hb_cxx_prove_mixed / hb_cxx_verify_rhs_mixed read each descriptor's fourteen raw
words and answer with the oracle's cxx restatement -- no GPU.

Three beats -- a 256-bit prime with S = 4, a 128-bit modulus with S = 3, a
1024-bit one with S = 10 -- interleaved in one call.

Reference: a storage node's loop of b.prove(...) over the challenges of many
owners (cxx/shacham_waters_private.cxx:731-789; one prime per Swizzle,
:596-624) and an auditor's loop of b.verify(...) (:791-842)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError
from test_cxx_pv_many import PvLib

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
# odd numbers of the right bit lengths: the oracle and the stand-in need no primality
P128 = (1 << 127) | 0x123456789abcdef0fedcba987654321
P1024 = (1 << 1023) | int.from_bytes(bytes(range(1, 128)), "big") | 1
BEATS = [(P256, 4), (P128, 3), (P1024, 10)]


def _w(p):
    return (p.bit_length() + 7) // 8


def _prove(p, S, key, chunks, vmax, tags, ntags, data):
    from oracle import oracle as O
    w = _w(p)
    mu, sg = O.cxx_prove(p, S, key, chunks, vmax, ntags, lambda k: int.from_bytes(tags[k * w:(k + 1) * w], "big"),
                         lambda off, n: data[off:off + n])
    return b"".join(m.to_bytes(w, "big") for m in mu), sg.to_bytes(w, "big")


def _rhs(p, S, fk, ak, nstate, ck, chunks, vmax, mub):
    from oracle import oracle as O
    w = _w(p)
    check_all = chunks >= nstate
    acc = 0
    for i in range(nstate if check_all else chunks):
        idx = i if check_all else O.cxx_prf_eval(ck, nstate, i)[0]
        acc += O.cxx_prf_eval(ck, vmax, i)[0] * O.cxx_prf_eval(fk, p, idx)[0]
    for j in range(S):
        acc += O.cxx_prf_eval(ak, p, j)[0] * int.from_bytes(mub[j * w:(j + 1) * w], "big")
    return (acc % p).to_bytes(w, "big")


class CxxMixedLib(PvLib):
    """PvLib's context and State AES, the single cxx prove and verify under any
    prime, and the two mixed calls reading each descriptor's raw words."""

    def hb_prove_range(self, h, pb, plen, sectors, key, klen, chunks, i0, i1, vmax, vlen, tags, ntags, data, length,
                       flags, mu_out, sg_out):
        from heartbeat_amd import _native
        assert flags & _native.HB_PRF_CXX and i0 == 0 and i1 >= chunks
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("prove", int(chunks), int(length)))
        blob = ctypes.string_at(self._addr(data), int(length)) if length else b""
        mu, sg = _prove(p, sectors, bytes(key[:klen]), int(chunks), int.from_bytes(bytes(vmax[:vlen]), "big"),
                        ctypes.string_at(self._addr(tags), int(ntags) * _w(p)), int(ntags), blob)
        ctypes.memmove(mu_out, mu, len(mu))
        ctypes.memmove(sg_out, sg, len(sg))
        return 0

    def hb_cxx_verify_rhs(self, h, pb, plen, sectors, fk, ak, klen, nstate, ck, cklen, chunks, vmax, vlen, mu, rhs_out):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("verify", int(nstate), int(chunks)))
        rhs = _rhs(p, sectors, bytes(fk[:klen]), bytes(ak[:klen]), int(nstate), bytes(ck[:cklen]), int(chunks),
                   int.from_bytes(bytes(vmax[:vlen]), "big"), bytes(mu[:sectors * _w(p)]))
        ctypes.memmove(rhs_out, rhs, len(rhs))
        return 0

    def hb_cxx_prove_mixed(self, h, descs, n, flags):
        seen = []
        for i in range(n):
            # p_be, p_len, sectors, key_len, then hb_prove_desc's ten words
            x = (ctypes.c_uint64 * 14).from_address(ctypes.addressof(descs[i]))
            p = int.from_bytes(ctypes.string_at(x[0], x[1]), "big")
            S, klen = int(x[2]), int(x[3])
            seen.append((p, S, klen))
            tags = ctypes.string_at(x[8], x[9] * _w(p))
            data = ctypes.string_at(x[10], x[11]) if x[11] else b""
            mu, sg = _prove(p, S, ctypes.string_at(x[4], klen), x[5], int.from_bytes(ctypes.string_at(x[6], x[7]), "big"),
                            tags, x[9], data)
            ctypes.memmove(x[12], mu, len(mu))
            ctypes.memmove(x[13], sg, len(sg))
        self.log.append(("prove_mixed", int(flags), seen))
        return 0

    def hb_cxx_verify_rhs_mixed(self, h, descs, n, flags):
        seen = []
        for i in range(n):
            # p_be, p_len, sectors, key_len, chal_key_len, then hb_verify_desc's nine words
            x = (ctypes.c_uint64 * 14).from_address(ctypes.addressof(descs[i]))
            p = int.from_bytes(ctypes.string_at(x[0], x[1]), "big")
            S, klen, cklen = int(x[2]), int(x[3]), int(x[4])
            seen.append((p, S, klen, cklen))
            rhs = _rhs(p, S, ctypes.string_at(x[5], klen), ctypes.string_at(x[6], klen), x[8], ctypes.string_at(x[7], cklen),
                       x[9], int.from_bytes(ctypes.string_at(x[10], x[11]), "big"), ctypes.string_at(x[12], S * _w(p)))
            ctypes.memmove(x[13], rhs, len(rhs))
        self.log.append(("verify_mixed", int(flags), seen))
        return 0

    # the PySwizzle mixed calls must not be what the cxx Swizzle reaches
    def hb_prove_mixed(self, *a):
        raise AssertionError("the cxx Swizzle called hb_prove_mixed")

    def hb_verify_rhs_mixed(self, *a):
        raise AssertionError("the cxx Swizzle called hb_verify_rhs_mixed")


@pytest.fixture
def swz():
    return importlib.import_module("heartbeat_amd.Swizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = CxxMixedLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


@pytest.fixture
def audit(lib, oracle, swz):
    """Three beats and nine files, beats interleaved: [(beat, blob, tag, state)]."""
    beats = [swz.Swizzle(sectors=S, prime=p) for p, S in BEATS]
    out = []
    for k in range(9):
        beat = beats[k % 3]
        p, S, w = beat.prime, beat.sectors, _w(beat.prime)
        blob = bytes((13 * k + i) & 0xff for i in range([0, 90, 700][k // 3] + 7 * k))
        state = swz.State()
        state.f_key, state.alpha_key = bytes([k + 1]) * 32, bytes([k + 101]) * 32
        sig = oracle.cxx_encode(p, S, state.f_key, state.alpha_key, blob)
        state.n = len(sig)
        state.encrypt(beat.k_enc, beat.k_mac)
        state = swz.State.fromdict(state.todict())          # as an auditor holds it: no keys in the clear
        out.append((beat, blob, swz.Tag._from_raw(memoryview(b"".join(t.to_bytes(w, "big") for t in sig)), w), state))
    return beats, out


def _pairs(proofs):
    return [(x.mu, x.sigma) for x in proofs]


def _chals(swz, audit, counts, klens=(32,)):
    return [swz.Challenge(n, beat.prime, bytes([k + 50]) * klens[k % len(klens)])
            for k, ((beat, _, _, _), n) in enumerate(zip(audit, counts))]


def test_prove_mixed_equals_loop_and_descriptors(lib, audit, swz, tmp_path):
    beats, files = audit
    counts = (1, 1, 0, 2, 1, 3, 9, 2, 1)                     # check_all, sampled and a zero proof
    chals = _chals(swz, files, counts, klens=(32, 16, 24, 32))
    path = tmp_path / "real.bin"
    path.write_bytes(files[7][1])
    fobjs = [io.BytesIO(blob) for _, blob, _, _ in files]
    fobjs[7] = open(str(path), "rb")
    try:
        fobjs[7].seek(5)
        fobjs[3].seek(11)
        items = [(beat.get_public(), f, c, tag) for (beat, _, tag, _), f, c in zip(files, fobjs, chals)]
        got = swz.Swizzle.prove_mixed(items)
        assert fobjs[7].tell() == 5 and fobjs[3].tell() == 11                   # positions restored
        (kind, flags, seen), = lib.log
        assert (kind, flags) == ("prove_mixed", 0)
        # the zero proof has no descriptor; every other carries its own item's prime, S and key length
        assert seen == [(b.prime, b.sectors, len(c.key)) for (b, _, c, _), n in zip(items, counts) if n]
        assert len({s[0] for s in seen}) == 3 and {s[2] for s in seen} == {16, 24, 32}
        del lib.log[:]
        want = [b.prove(f, c, t) for b, f, c, t in items]
        assert [e[0] for e in lib.log] == ["prove"] * 8
        assert _pairs(got) == _pairs(want)
        assert all(isinstance(g, swz.Proof) for g in got)
        assert (got[2].mu, got[2].sigma) == ([0] * beats[2].sectors, 0)
        assert _pairs(swz.Swizzle.prove_mixed(iter(items))) == _pairs(want)     # any iterable
    finally:
        fobjs[7].close()
    assert swz.Swizzle.prove_mixed([]) == []


def test_prove_mixed_error_order_and_sharding(lib, audit, swz, monkeypatch):
    beats, files = audit
    chals = _chals(swz, files, (1, 2, 0, 2, 1, 3, 2, 2, 1))
    items = [(beat, io.BytesIO(blob), c, tag) for (beat, blob, tag, _), c in zip(files, chals)]
    # an empty tag with chunks == 0: the cxx prove raises before it looks at the challenge
    items[2] = items[2][:3] + (swz.Tag(),)
    with pytest.raises(HeartbeatError) as e:
        swz.Swizzle.prove_mixed(items)
    with pytest.raises(HeartbeatError) as e1:
        [b.prove(f, c, t) for b, f, c, t in items]
    assert str(e.value) == str(e1.value) == "tag is empty"
    assert lib.log == [("prove", 1, len(files[0][1])), ("prove", 2, len(files[1][1]))]   # the loop got that far; the batch: nothing
    del lib.log[:]
    bad = swz.Swizzle(sectors=0, prime=P256)
    with pytest.raises(HeartbeatError) as e:
        swz.Swizzle.prove_mixed(items[:1] + [(bad,) + items[0][1:]])
    assert "sectors must be positive" in str(e.value) and lib.log == []
    # challenges that prove() would shard over two GPUs go through prove()
    from heartbeat_amd import multi
    monkeypatch.setattr(multi, "_devices", [0, 0])
    monkeypatch.setattr(multi, "MIN_SHARD_CHUNKS", 6)
    items = [(beat, io.BytesIO(blob), c, tag) for (beat, blob, tag, _), c in zip(files, chals)][3:7]
    items[2][2].chunks = 12
    monkeypatch.setattr(multi, "prove_shards", lambda *a: ([7], 7))
    got = swz.Swizzle.prove_mixed(items)
    assert [e[0] for e in lib.log] == ["prove_mixed"] and len(lib.log[0][2]) == 3
    assert (got[2].mu, got[2].sigma) == ([7], 7)


def test_verify_mixed_equals_loop(lib, audit, swz):
    beats, files = audit
    counts = (1, 1, 0, 2, 1, 3, 9, 2, 1)
    chals = _chals(swz, files, counts)
    items = [(beat, io.BytesIO(blob), c, tag) for (beat, blob, tag, _), c in zip(files, chals)]
    proofs = swz.Swizzle.prove_mixed(items)
    del lib.log[:]
    vit = [(beat, q, c, state) for (beat, _, _, state), q, c in zip(files, proofs, chals)]
    got = swz.Swizzle.verify_mixed(vit)
    (kind, flags, seen), = lib.log
    assert (kind, flags) == ("verify_mixed", 0)
    assert seen == [(b.prime, b.sectors, 32, 32) for b, _, _, _ in vit]
    assert got == [True] * 9
    del lib.log[:]
    assert [b.verify(q, c, s) for b, q, c, s in vit] == got and [e[0] for e in lib.log] == ["verify"] * 9
    # tampered, wrong types, a short mu, a state under another beat's keys
    proofs[4].mu[1] ^= 1
    short = swz.Proof()
    short.mu, short.sigma = proofs[0].mu[:-1], proofs[0].sigma
    vit2 = list(vit) + [(beats[0], "no proof", chals[0], files[0][3]), (beats[0], short, chals[0], files[0][3]),
                        (beats[1], proofs[0], chals[0], files[0][3])]
    want = [k != 4 for k in range(9)] + [None, False, False]
    del lib.log[:]
    assert swz.Swizzle.verify_mixed(vit2) == want
    assert [e[0] for e in lib.log] == ["verify_mixed"] and len(lib.log[0][2]) == 9
    assert [b.verify(q, c, s) for b, q, c, s in vit2] == want
    assert swz.Swizzle.verify_mixed([]) == []
    # a state without chunks under a challenge: the loop's error, before any call
    state = swz.State()
    state.f_key, state.alpha_key, state.n = b"f" * 32, b"a" * 32, 0
    state.encrypt(beats[2].k_enc, beats[2].k_mac)
    del lib.log[:]
    with pytest.raises(HeartbeatError) as e:
        swz.Swizzle.verify_mixed(vit[:2] + [(beats[2], proofs[2], swz.Challenge(3, P1024, b"k" * 32), state)])
    assert str(e.value) == "state has no chunks" and lib.log == []


def test_module_functions_and_the_pyswizzle_callers(lib, audit, swz, oracle):
    from heartbeat_amd import _many
    beats, files = audit
    beat, blob, tag, _ = files[7]
    p, S, w = beat.prime, beat.sectors, _w(beat.prime)
    ck = b"c" * 24
    got = swz.prove_files_mixed([(p, S, ck, 2, p, tag, io.BytesIO(blob)), (P256, 4, b"k" * 16, -2, 77, files[0][2], b"")])
    mu, sg = oracle.cxx_prove(p, S, ck, 2, p, len(tag), lambda k: tag.sigma[k], lambda off, n: blob[off:off + n])
    assert got[0] == (mu, sg) and got[1] == ([0] * 4, 0)
    assert lib.log[-1][0] == "prove_mixed" and lib.log[-1][2] == [(p, S, 24), (P256, 4, 16)]
    fk, ak = b"f" * 32, b"a" * 32
    rhs = swz.verify_rhs_mixed([(p, S, fk, ak, 5, ck, 2, p, mu)])
    assert rhs == [int.from_bytes(_rhs(p, S, fk, ak, 5, ck, 2, p, b"".join(m.to_bytes(w, "big") for m in mu)), "big")]
    assert lib.log[-1][0] == "verify_mixed" and lib.log[-1][2] == [(p, S, 32, 24)]
    n = len(lib.log)
    # the cxx policy: exactly `sectors` mu values
    with pytest.raises(HeartbeatError) as e:
        swz.verify_rhs_mixed([(p, S, fk, ak, 5, ck, 2, p, mu + [1])])
    assert str(e.value) == "proof has %d mu values, not %d" % (S + 1, S)
    with pytest.raises(HeartbeatError):
        swz.prove_files_mixed([(p, S, ck, 3, p, swz.Tag(), b"")])
    with pytest.raises(HeartbeatError):
        swz.prove_files_mixed([(p, 0, ck, 3, p, tag, b"")])
    assert swz.prove_files_mixed([]) == [] and swz.verify_rhs_mixed([]) == [] and len(lib.log) == n
    # the defaults are the PySwizzle callers': hb_prove_mixed / hb_verify_rhs_mixed, more mu values allowed
    with pytest.raises(AssertionError) as e:
        _many.prove_files_mixed([(p, S, ck, 2, p, tag, io.BytesIO(blob))])
    assert "hb_prove_mixed" in str(e.value)
    with pytest.raises(AssertionError) as e:
        _many.verify_rhs_mixed([(p, S, fk, ak, 5, ck, 2, p, mu + [1])])
    assert "hb_verify_rhs_mixed" in str(e.value)
