"""CPU tests of the batched cxx prove's and verify's Python layer
(heartbeat_amd.Swizzle: prove_files, verify_rhs_many, Swizzle.prove_many and
Swizzle.verify_many = heartbeat.Heartbeat()'s) over a small stand-in for
libhbswizzle.so whose entry points delegate to the oracle's cxx restatement --
no GPU.

Reference: a caller's loops over Swizzle.prove and Swizzle.verify
(cxx/shacham_waters_private.cxx:731-789, 791-842)."""
import ctypes
import importlib
import io

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
W = 32
C = 32 * S


class PvLib(object):
    """The entry points Swizzle.prove / verify and the batch helpers reach: a
    context, the two batched calls and the two single calls over the oracle,
    and a reversible stand-in for the State's AES.  `log` records every call
    that would run on the GPU."""

    def __init__(self):
        self.log = []

    def hb_ctx_create(self, device, ref):
        ref._obj.value = 1 + device
        return 0

    def hb_ctx_destroy(self, h):
        pass

    def hb_last_error(self, h):
        return b"stand-in"

    def hb_device_count(self, ref):
        ref._obj.value = 1
        return 0

    def hb_aes_cfb128(self, key, klen, iv, data, out, n, encrypt):
        pad = (bytes(key[:klen]) + bytes(iv[:16])) * (n // 16 + 1)
        ctypes.memmove(out, bytes(a ^ b for a, b in zip(bytes(data[:n]), pad)), n)
        return 0

    @staticmethod
    def _addr(x):
        return x if isinstance(x, int) or x is None else getattr(x, "value", None) or ctypes.addressof(x)

    @staticmethod
    def _prove(p, sectors, key, chunks, vmax, tags, ntags, data):
        from oracle import oracle as O
        mu, sg = O.cxx_prove(p, sectors, key, chunks, vmax, ntags,
                             lambda k: int.from_bytes(tags[k * W:(k + 1) * W], "big"),
                             lambda off, n: data[off:off + n])
        return b"".join(m.to_bytes(W, "big") for m in mu), sg.to_bytes(W, "big")

    @staticmethod
    def _rhs(p, sectors, fk, ak, nstate, ck, chunks, vmax, mub):
        from oracle import oracle as O
        check_all = chunks >= nstate
        acc = 0
        for i in range(nstate if check_all else chunks):
            idx = i if check_all else O.cxx_prf_eval(ck, nstate, i)[0]
            acc += O.cxx_prf_eval(ck, vmax, i)[0] * O.cxx_prf_eval(fk, p, idx)[0]
        for j in range(sectors):
            acc += O.cxx_prf_eval(ak, p, j)[0] * int.from_bytes(mub[j * W:(j + 1) * W], "big")
        return (acc % p).to_bytes(W, "big")

    def hb_cxx_prove_many(self, h, pb, plen, sectors, klen, descs, n, flags):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("prove_many", int(n), int(klen), int(flags)))
        for i in range(n):
            # the struct's raw words: chal_key, chunks, vmax_be, vmax_len, tags, ntags, data, len, mu_out, sigma_out
            w = (ctypes.c_uint64 * 10).from_address(ctypes.addressof(descs[i]))
            key, vmax = ctypes.string_at(w[0], klen), int.from_bytes(ctypes.string_at(w[2], w[3]), "big")
            tags = ctypes.string_at(w[4], w[5] * W)
            data = ctypes.string_at(w[6], w[7]) if w[7] else b""
            mu, sg = self._prove(p, sectors, key, w[1], vmax, tags, w[5], data)
            ctypes.memmove(w[8], mu, len(mu))
            ctypes.memmove(w[9], sg, len(sg))
        return 0

    def hb_prove_range(self, h, pb, plen, sectors, key, klen, chunks, i0, i1, vmax, vlen, tags, ntags, data, length,
                       flags, mu_out, sg_out):
        from heartbeat_amd import _native
        assert flags & _native.HB_PRF_CXX and i0 == 0 and i1 >= chunks
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("prove", int(chunks), int(length)))
        blob = ctypes.string_at(self._addr(data), int(length)) if length else b""
        mu, sg = self._prove(p, sectors, bytes(key[:klen]), int(chunks), int.from_bytes(bytes(vmax[:vlen]), "big"),
                             ctypes.string_at(self._addr(tags), int(ntags) * W), int(ntags), blob)
        ctypes.memmove(mu_out, mu, len(mu))
        ctypes.memmove(sg_out, sg, len(sg))
        return 0

    def hb_cxx_verify_rhs_many(self, h, pb, plen, sectors, klen, cklen, descs, n, flags):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("verify_many", int(n), int(klen), int(cklen), int(flags)))
        for i in range(n):
            # f_key, alpha_key, chal_key, state_chunks, chunks, vmax_be, vmax_len, mu, rhs_out
            w = (ctypes.c_uint64 * 9).from_address(ctypes.addressof(descs[i]))
            rhs = self._rhs(p, sectors, ctypes.string_at(w[0], klen), ctypes.string_at(w[1], klen), w[3],
                            ctypes.string_at(w[2], cklen), w[4], int.from_bytes(ctypes.string_at(w[5], w[6]), "big"),
                            ctypes.string_at(w[7], sectors * W))
            ctypes.memmove(w[8], rhs, W)
        return 0

    def hb_cxx_verify_rhs(self, h, pb, plen, sectors, fk, ak, klen, nstate, ck, cklen, chunks, vmax, vlen, mu, rhs_out):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        self.log.append(("verify", int(nstate), int(chunks)))
        rhs = self._rhs(p, sectors, bytes(fk[:klen]), bytes(ak[:klen]), int(nstate), bytes(ck[:cklen]), int(chunks),
                        int.from_bytes(bytes(vmax[:vlen]), "big"), bytes(mu[:sectors * W]))
        ctypes.memmove(rhs_out, rhs, W)
        return 0


@pytest.fixture
def swz():
    return importlib.import_module("heartbeat_amd.Swizzle")


@pytest.fixture
def lib(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = PvLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])
    return fake


@pytest.fixture
def audit(lib, oracle, swz):
    """A Swizzle, five files with their tags and states (made over the oracle)."""
    beat = swz.Swizzle(sectors=S, prime=P256)
    blobs = [b"", b"q" * (C - 1), b"r" * C, bytes(range(200)) * 5, b"tail" * 399]
    enc = []
    for k, blob in enumerate(blobs):
        state = swz.State()
        state.f_key, state.alpha_key = bytes([k + 1]) * 32, bytes([k + 101]) * 32
        sig = oracle.cxx_encode(P256, S, state.f_key, state.alpha_key, blob)
        state.n = len(sig)
        state.encrypt(beat.k_enc, beat.k_mac)
        state = swz.State.fromdict(state.todict())          # as an auditor holds it: no keys in the clear
        enc.append((swz.Tag._from_raw(memoryview(b"".join(t.to_bytes(W, "big") for t in sig)), W), state))
    return beat, blobs, enc


def _chal(swz, chunks, key):
    return swz.Challenge(chunks, P256, key)


def test_prove_many_and_verify_many_equal_the_loops(lib, audit, swz, tmp_path):
    beat, blobs, enc = audit
    pub = beat.get_public()
    chals = [_chal(swz, n, bytes([k + 50]) * 32) for k, n in enumerate((1, 0, 2, 3, 13))]   # 0: a zero proof
    path = tmp_path / "real.bin"
    path.write_bytes(blobs[4])
    files = [io.BytesIO(b) for b in blobs[:4]] + [open(str(path), "rb")]
    try:
        for f, k in zip(files, (0, 5, 3, 100, 7)):
            f.seek(k)
        proofs = pub.prove_many([(f, c, tag) for f, c, (tag, _) in zip(files, chals, enc)])
        assert [f.tell() for f in files] == [0, 5, 3, 100, 7]                  # positions restored
    finally:
        files[4].close()
    assert lib.log == [("prove_many", 4, 32, 0)]                                 # the zero proof costs nothing
    del lib.log[:]
    loop = [pub.prove(io.BytesIO(b), c, tag) for b, c, (tag, _) in zip(blobs, chals, enc)]
    assert [x[0] for x in lib.log] == ["prove"] * 4
    assert [(q.mu, q.sigma) for q in proofs] == [(q.mu, q.sigma) for q in loop]
    assert proofs[1].mu == [0] * S and proofs[1].sigma == 0
    del lib.log[:]
    items = [(q, c, state) for q, c, (_, state) in zip(proofs, chals, enc)]
    got = beat.verify_many(items)
    assert lib.log == [("verify_many", 5, 32, 32, 0)]
    assert got == [beat.verify(*it) for it in items]
    # honest proofs verify where the challenge covers the tags it sampled
    assert got[0] is True and got[4] is True
    assert all(state.encrypted and not state.f_key for _, _, state in items)    # the caller's states are untouched


def test_verify_many_none_false_and_raise(lib, audit, swz):
    beat, blobs, enc = audit
    pub = beat.get_public()
    chal = _chal(swz, 3, b"\x44" * 32)
    proof = pub.prove(io.BytesIO(blobs[3]), chal, enc[3][0])
    short = swz.Proof()
    short.mu, short.sigma = proof.mu[:-1], proof.sigma
    forged = enc[3][1]._copy()
    forged._raw = forged._raw[:-1] + bytes([forged._raw[-1] ^ 1])
    items = [(proof, chal, enc[3][1]), ("no proof", chal, enc[3][1]), (short, chal, enc[3][1]),
             (proof, chal, forged), (proof, chal, enc[3][1])]
    del lib.log[:]
    assert beat.verify_many(items) == [True, None, False, False, True]
    assert lib.log == [("verify_many", 2, 32, 32, 0)]
    del lib.log[:]
    assert [beat.verify(*it) for it in items] == [True, None, False, False, True]
    # a state without chunks: raised as the loop raises it, before any GPU work
    empty = swz.State()
    empty.f_key, empty.alpha_key, empty.n = b"f" * 32, b"a" * 32, 0
    empty.encrypt(beat.k_enc, beat.k_mac)
    del lib.log[:]
    with pytest.raises(HeartbeatError, match="state has no chunks"):
        beat.verify_many(items + [(proof, chal, empty)])
    assert lib.log == []
    with pytest.raises(HeartbeatError, match="state has no chunks"):
        beat.verify(proof, chal, empty)


def test_prove_many_raises_before_any_gpu_work(lib, audit, swz):
    beat, blobs, enc = audit
    chal = _chal(swz, 2, b"\x55" * 32)
    files = [io.BytesIO(b) for b in blobs[:3]]
    files[0].seek(0)
    items = [(files[0], chal, enc[0][0]), (files[1], chal, swz.Tag()), (files[2], chal, enc[2][0])]
    del lib.log[:]
    with pytest.raises(HeartbeatError, match="tag is empty"):
        beat.prove_many(items)
    assert lib.log == []
    # an empty tag raises even with chunks <= 0, as prove() does
    with pytest.raises(HeartbeatError, match="tag is empty"):
        beat.prove_many([(files[1], _chal(swz, 0, b"k" * 32), swz.Tag())])
    with pytest.raises(HeartbeatError, match="tag is empty"):
        beat.prove(files[1], _chal(swz, 0, b"k" * 32), swz.Tag())
    for bad in (swz.Swizzle(sectors=0, prime=P256), swz.Swizzle(sectors=S, prime=127)):
        with pytest.raises(HeartbeatError):
            bad.prove_many(items[:1])
    with pytest.raises(HeartbeatError):
        swz.prove_files(P256, S, [(b"k" * 32, 1, P256, enc[0][0], files[0]), (b"k" * 16, 1, P256, enc[2][0], files[2])])
    with pytest.raises(HeartbeatError):
        swz.verify_rhs_many(P256, S, [(b"f" * 32, b"a" * 32, 3, b"k" * 32, 1, P256, [1] * (S - 1))])
    with pytest.raises(HeartbeatError):
        swz.verify_rhs_many(P256, S, [(b"f" * 32, b"a" * 16, 3, b"k" * 32, 1, P256, [1] * S)])
    assert lib.log == []
    assert swz.prove_files(P256, S, []) == [] and swz.verify_rhs_many(P256, S, []) == []
    assert beat.prove_many([]) == [] and beat.verify_many([]) == [] and lib.log == []


def test_majority_rule_and_order(lib, audit, swz):
    """Items whose challenge key length differs from the majority's go through
    the single methods; the results keep the items' order."""
    beat, blobs, enc = audit
    pub = beat.get_public()
    klens = (32, 16, 32, 32, 16)
    chals = [_chal(swz, 2, bytes([k + 60]) * n) for k, n in enumerate(klens)]
    del lib.log[:]
    proofs = pub.prove_many([(io.BytesIO(b), c, tag) for b, c, (tag, _) in zip(blobs, chals, enc)])
    assert lib.log[0] == ("prove_many", 3, 32, 0) and [x[0] for x in lib.log[1:]] == ["prove", "prove"]
    loop = [pub.prove(io.BytesIO(b), c, tag) for b, c, (tag, _) in zip(blobs, chals, enc)]
    assert [(q.mu, q.sigma) for q in proofs] == [(q.mu, q.sigma) for q in loop]
    assert len({q.sigma for q in proofs}) > 1
    items = [(q, c, state) for q, c, (_, state) in zip(proofs, chals, enc)]
    del lib.log[:]
    got = beat.verify_many(items)
    assert lib.log[0] == ("verify_many", 3, 32, 32, 0) and [x[0] for x in lib.log[1:]] == ["verify", "verify"]
    assert got == [beat.verify(*it) for it in items]


def test_below_the_minimum_the_single_methods_run(lib, audit, swz, monkeypatch):
    beat, blobs, enc = audit
    pub = beat.get_public()
    assert swz.CXX_PROVE_MANY_MIN >= 1 and swz.CXX_VERIFY_MANY_MIN >= 1
    monkeypatch.setattr(swz, "CXX_PROVE_MANY_MIN", 3)
    monkeypatch.setattr(swz, "CXX_VERIFY_MANY_MIN", 3)
    chals = [_chal(swz, 2, bytes([k + 70]) * 32) for k in range(3)]
    trio = [(io.BytesIO(b), c, tag) for b, c, (tag, _) in zip(blobs[2:5], chals, enc[2:5])]
    del lib.log[:]
    two = pub.prove_many(trio[:2])
    assert [x[0] for x in lib.log] == ["prove", "prove"]
    del lib.log[:]
    three = pub.prove_many(trio)
    assert lib.log == [("prove_many", 3, 32, 0)]
    assert [(q.mu, q.sigma) for q in two] == [(q.mu, q.sigma) for q in three[:2]]
    items = [(q, c, state) for q, c, (_, state) in zip(three, chals, enc[2:5])]
    del lib.log[:]
    a = beat.verify_many(items[:2])
    assert [x[0] for x in lib.log] == ["verify", "verify"]
    del lib.log[:]
    b = beat.verify_many(items)
    assert lib.log == [("verify_many", 3, 32, 32, 0)] and a == b[:2]


def test_reexported_through_heartbeat(swz):
    import heartbeat
    hb = importlib.import_module("heartbeat.Swizzle")
    assert heartbeat.Heartbeat is hb.Swizzle is swz.Swizzle
    assert hasattr(heartbeat.Heartbeat, "prove_many") and hasattr(heartbeat.Heartbeat, "verify_many")


def test_symbols_are_bound():
    from heartbeat_amd import _native
    names = {name: args for name, _, args in _native.SIGNATURES}
    assert names["hb_cxx_prove_many"] == names["hb_prove_many"]
    assert names["hb_cxx_verify_rhs_many"] == names["hb_verify_rhs_many"]
