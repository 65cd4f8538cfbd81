"""CPU tests of the batched verify's Python layer (heartbeat_amd.PySwizzle:
verify_rhs_many, PySwizzle.verify_many) over a small stand-in for
libhbswizzle.so whose hb_verify_rhs / hb_verify_rhs_many compute the
right-hand side with the CPU oracle's KeyedPRF -- no GPU.

Reference: a caller's loop over PySwizzle.py:372-395 (verify decrypts the
state, :373, and compares sigma with sum v_i F(idx_i) + sum alpha_j mu_j,
:381-394)."""
import ctypes
import importlib

import pytest

from heartbeat_amd.exc import HeartbeatError

P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)
S = 4
C = 32 * S
KEY = b"K" * 32


def _rhs(p, sectors, fk, ak, nstate, ck, chunks, vmax, mu):
    """PySwizzle.py:381-394 with the oracle's KeyedPRF."""
    from oracle import oracle as O
    rhs = 0
    for i in range(chunks):
        rhs += O.prf_eval(ck, vmax, i) * O.prf_eval(fk, p, O.prf_eval(ck, nstate, i))
    for j in range(sectors):
        rhs += O.prf_eval(ak, p, j) * mu[j]
    return rhs % p


class VerifyLib(object):
    """The entry points verify and verify_rhs_many reach: a context, the
    single hb_verify_rhs and hb_verify_rhs_many reading each descriptor's
    nine raw words."""

    def __init__(self):
        self.calls = []
        self.single = 0

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

    def hb_verify_rhs(self, h, pb, plen, sectors, fk, ak, klen, nstate, ck, cklen, chunks, vmax, vlen, mub, rhs):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.single += 1
        mu = [int.from_bytes(mub[j * w:(j + 1) * w], "big") for j in range(sectors)]
        r = _rhs(p, sectors, fk[:klen], ak[:klen], nstate, ck[:cklen], chunks,
                 int.from_bytes(vmax[:vlen], "big"), mu)
        ctypes.memmove(rhs, r.to_bytes(w, "big"), w)
        return 0

    def hb_verify_rhs_many(self, h, pb, plen, sectors, klen, cklen, descs, n, flags):
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        self.calls.append((int(n), int(klen), int(cklen), int(flags)))
        for i in range(n):
            # the struct's raw words: f_key, alpha_key, chal_key, state_chunks,
            # chunks, vmax_be, vmax_len, mu, rhs_out
            x = (ctypes.c_uint64 * 9).from_address(ctypes.addressof(descs[i]))
            fk, ak, ck = ctypes.string_at(x[0], klen), ctypes.string_at(x[1], klen), ctypes.string_at(x[2], cklen)
            vmax = int.from_bytes(ctypes.string_at(x[5], x[6]), "big")
            mub = ctypes.string_at(x[7], sectors * w)
            mu = [int.from_bytes(mub[j * w:(j + 1) * w], "big") for j in range(sectors)]
            r = _rhs(p, sectors, fk, ak, x[3], ck, x[4], vmax, mu)
            ctypes.memmove(x[8], r.to_bytes(w, "big"), w)
        return 0


@pytest.fixture
def pys():
    return importlib.import_module("heartbeat_amd.PySwizzle.PySwizzle")


@pytest.fixture
def many(monkeypatch):
    from heartbeat_amd import _native, multi
    fake = VerifyLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(multi, "_devices", [0])

    def xor_cfb8(key, iv, data, encrypt):                      # a reversible stand-in for hb_aes_cfb8
        pad = (bytes(key) + bytes(iv)) * (len(data) // 16 + 1)
        return bytes(a ^ b for a, b in zip(bytes(data), pad))

    monkeypatch.setattr(_native, "aes_cfb8", xor_cfb8)
    return fake


def _items(pys, oracle, n, klen=32, cklen=32, first=0):
    """n honest (proof, chal, state) over files of a few hundred bytes."""
    out = []
    for k in range(first, first + n):
        data = bytes((7 * k + i) & 0xff for i in range(300 + 97 * (k % 5)))
        fk, ak, ck = bytes([k + 1]) * klen, bytes([0x80 + k]) * klen, bytes([0x40 + k]) * cklen
        tags = oracle.encode(P256, S, fk, ak, data)
        chunks = len(tags)
        mu, sigma = oracle.prove(P256, S, ck, chunks, P256, tags, data)
        proof = pys.Proof()
        proof.mu, proof.sigma = mu, sigma
        state = pys.State(fk, ak, chunks)
        state.encrypt(KEY)
        out.append((proof, pys.Challenge(chunks, P256, ck), state))
    return out


def test_verify_many_equals_loop_of_verify(many, oracle, pys):
    beat = pys.PySwizzle(S, KEY, P256)
    items = _items(pys, oracle, 5)
    items[1][0].mu[2] ^= 1                                     # a tampered mu
    items[3][0].sigma = (items[3][0].sigma + 1) % P256         # a tampered sigma
    want = [beat.verify(*it) for it in items]
    assert want == [True, False, True, False, True]
    assert many.single == 5 and many.calls == []
    got = beat.verify_many(items)
    assert got == want
    assert many.calls == [(5, 32, 32, 0)]                      # one call, the right counts and key lengths
    assert many.single == 5                                    # and no single call beside it
    assert beat.verify_many(iter(items)) == want               # any iterable


def test_verify_rhs_many_values(many, oracle, pys):
    items = [(b"f" * 16, b"a" * 16, 9, b"c" * 24, 3, 1000, [1, 2, 3, 4]),
             (b"g" * 16, b"b" * 16, 1, b"d" * 24, 0, 77, [5, 6, 7, P256 + 8, 99])]
    got = pys.verify_rhs_many(P256, S, items)
    assert many.calls == [(2, 16, 24, 0)]
    assert got[0] == _rhs(P256, S, b"f" * 16, b"a" * 16, 9, b"c" * 24, 3, 1000, [1, 2, 3, 4])
    assert got[1] == _rhs(P256, S, b"g" * 16, b"b" * 16, 1, b"d" * 24, 0, 1, [5, 6, 7, 8])   # mu mod p, S of them
    with pytest.raises(HeartbeatError):
        pys.verify_rhs_many(P256, S, [items[0], (b"g" * 32, b"b" * 32, 1, b"d" * 24, 0, 77, [0] * S)])
    with pytest.raises(HeartbeatError):
        pys.verify_rhs_many(P256, S, [items[0], (b"g" * 16, b"b" * 16, 1, b"d" * 32, 0, 77, [0] * S)])
    with pytest.raises(HeartbeatError):
        pys.verify_rhs_many(P256, S, [(b"g" * 16, b"b" * 16, 1, b"d" * 32, 0, 77, [0] * (S - 1))])
    with pytest.raises(HeartbeatError):
        pys.verify_rhs_many(P256, 0, items)
    assert len(many.calls) == 1


def test_bad_item_raises_before_any_library_call(many, oracle, pys):
    beat = pys.PySwizzle(S, KEY, P256)
    items = _items(pys, oracle, 3)
    items[1][2].hmac = bytes(32)                               # a bad signature in the middle
    with pytest.raises(HeartbeatError) as e:
        beat.verify_many(items)
    assert "Signature invalid" in str(e.value)
    with pytest.raises(HeartbeatError) as e1:
        [beat.verify(*it) for it in items]
    assert str(e1.value) == str(e.value)
    assert many.calls == []

    items = _items(pys, oracle, 3)
    items[2][0].mu = items[2][0].mu[:S - 1]                    # too few mu values
    with pytest.raises(HeartbeatError) as e:
        beat.verify_many(items)
    assert "fewer than %d mu values" % S in str(e.value)
    items = _items(pys, oracle, 2)
    items[0][2].decrypt(KEY)
    items[0][2].chunks = 0                                     # a state without chunks
    items[0][2].hmac = items[0][2].get_hmac(KEY)
    with pytest.raises(HeartbeatError) as e:
        beat.verify_many(items)
    assert "state has no chunks" in str(e.value)
    assert many.calls == []


def test_mixed_key_lengths(many, oracle, pys):
    beat = pys.PySwizzle(S, KEY, P256)
    items = _items(pys, oracle, 3) + _items(pys, oracle, 1, klen=16, first=3) + \
        _items(pys, oracle, 1, cklen=24, first=4) + _items(pys, oracle, 1, first=5)
    items[3][0].mu[0] ^= 2
    items[5][0].mu[1] ^= 4
    got = beat.verify_many(items)
    assert got == [True, True, True, False, True, False]
    assert many.calls == [(4, 32, 32, 0)]                      # the majority in one call
    assert many.single == 2                                    # the others through verify()
    assert got == [beat.verify(*it) for it in items]


def test_empty_list_makes_no_library_call(many, pys):
    assert pys.PySwizzle(S, KEY, P256).verify_many([]) == []
    assert pys.verify_rhs_many(P256, S, []) == []
    assert many.calls == [] and many.single == 0


def test_zero_chunk_challenge(many, oracle, pys):
    beat = pys.PySwizzle(S, KEY, P256)
    (proof, chal, state), = _items(pys, oracle, 1)
    chal.chunks = 0
    proof.sigma = _rhs(P256, S, bytes([1]) * 32, bytes([0x80]) * 32, 1, b"", 0, 1, proof.mu)
    assert beat.verify_many([(proof, chal, state)]) == [beat.verify(proof, chal, state)] == [True]


def test_single_item_goes_through_verify(many, oracle, pys):
    """Below VERIFY_MANY_MIN items the batch's two launches lose to the single
    fused launch: verify() is used."""
    assert pys.VERIFY_MANY_MIN == 2
    beat = pys.PySwizzle(S, KEY, P256)
    items = _items(pys, oracle, 1)
    assert beat.verify_many(items) == [True]
    assert many.calls == [] and many.single == 1


def test_reexported_through_heartbeat(pys):
    hb = importlib.import_module("heartbeat.PySwizzle.PySwizzle")
    assert hb.verify_rhs_many is pys.verify_rhs_many
    assert hasattr(hb.PySwizzle, "verify_many")
