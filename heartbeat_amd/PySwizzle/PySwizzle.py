"""Drop-in for heartbeat.PySwizzle (heartbeat/PySwizzle/PySwizzle.py) whose
encode / prove / verify run on an MI355X through libhbswizzle.so.

Same class names, constructor arguments, method signatures, defaults,
``todict`` schemas and error messages as the reference:

    Challenge(chunks, v_max, key)                 PySwizzle.py:33-64
    Tag()  .sigma                                 PySwizzle.py:67-91
    State(f_key, alpha_key, chunks=0, ...)        PySwizzle.py:94-195
    Proof() .mu .sigma                            PySwizzle.py:198-224
    PySwizzle(sectors=10, key=None, prime=None, primebits=1024)
        encode(file) -> (Tag, State)              PySwizzle.py:279-314
        encode_many(files) -> [(Tag, State)]      a loop over :279-311, one GPU call
        gen_challenge(state) -> Challenge         PySwizzle.py:316-331
        prove(file, chal, tag) -> Proof           PySwizzle.py:333-370
        verify(proof, chal, state) -> bool        PySwizzle.py:372-395
        verify_many(items) -> [bool]              a loop over :372-395, one GPU call
        encode_blocks / update / update_file / update_many, patch_tag (static)
                                                  the body of :296-309 for listed blocks only
        prove_mixed(items) / verify_mixed(items)  (static) the same for any mix of beats

Tags produced by encode keep their fixed-width big-endian image (``Tag.raw``)
so prove can hand them to the GPU without converting 2^27 Python ints; the
``sigma`` list is materialised on first access.
"""
import copy
import ctypes
import hashlib
import hmac as _hmac
import os

import numpy as np

from .. import _blocks, _many, _native, multi
from .._filebuf import FileBuffer
from ..exc import HeartbeatError
from ..primes import getPrimes
from ..util import KeyedPRF, hb_decode, hb_encode

__all__ = ["KeyedPRF", "Challenge", "Tag", "State", "Proof", "PySwizzle", "getPrime", "getPrimes"]

AES_BLOCK = 16


def _random_bytes(n):
    return os.urandom(n)


# ---------------------------------------------------------------- primes
_SMALL_PRIMES = [q for q in range(3, 2000, 2) if all(q % d for d in range(3, int(q ** 0.5) + 1, 2))]


def _is_probable_prime(n, rounds=40):
    if n < 2:
        return False
    if n in (2, 3):
        return True
    if n % 2 == 0:
        return False
    for q in _SMALL_PRIMES:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for _ in range(rounds):
        a = 2 + int.from_bytes(os.urandom((n.bit_length() + 7) // 8 + 8), "big") % (n - 3)
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def getPrime(bits):
    """A random prime of exactly `bits` bits (Crypto.Util.number.getPrime)."""
    if bits < 2:
        raise HeartbeatError("prime size must be at least 2 bits")
    while True:
        x = int.from_bytes(os.urandom((bits + 7) // 8), "big")
        x &= (1 << bits) - 1
        x |= (1 << (bits - 1)) | 1
        if _is_probable_prime(x):
            return x


# ---------------------------------------------------------------- data types
class Challenge(object):
    """A challenge: check `chunks` blocks drawn with `key`, coefficients < v_max."""

    def __init__(self, chunks, v_max, key):
        self.chunks = chunks
        self.v_max = v_max
        self.key = key

    def todict(self):
        return {"chunks": self.chunks, "v_max": self.v_max, "key": hb_encode(self.key)}

    @staticmethod
    def fromdict(dict):
        return Challenge(dict["chunks"], dict["v_max"], hb_decode(dict["key"]))


class Tag(object):
    """The file tag: one value sigma_i < p per block."""

    def __init__(self):
        self._sigma = list()
        self._raw = None      # fixed-width big-endian image from encode
        self._width = 0

    @classmethod
    def _from_raw(cls, raw, width):
        t = cls()
        t._sigma = None
        t._raw = raw
        t._width = width
        return t

    @classmethod
    def _from_sigma(cls, sigma):
        t = cls()
        t.sigma = sigma
        return t

    @property
    def sigma(self):
        if self._sigma is None:
            w, raw = self._width, bytes(self._raw)
            self._sigma = [int.from_bytes(raw[i:i + w], "big") for i in range(0, len(raw), w)]
        return self._sigma

    @sigma.setter
    def sigma(self, value):
        self._sigma = value
        self._raw = None
        self._width = 0

    def __len__(self):
        if self._sigma is None:
            return len(self._raw) // self._width
        return len(self._sigma)

    def raw(self, p):
        """Fixed-width big-endian image of the tag values (mod p when a value
        does not fit the width -- equal in every use, which is mod p)."""
        w = _native.width_of(p)
        if self._raw is not None and self._width == w and self._sigma is None:
            return self._raw
        top = 1 << (8 * w)
        return b"".join((s if 0 <= s < top else s % p).to_bytes(w, "big") for s in self.sigma)

    def __getstate__(self):
        # the encode image is a memoryview over the GPU output array: pickle bytes
        d = dict(self.__dict__)
        if d.get("_raw") is not None:
            d["_raw"] = bytes(d["_raw"])
        return d

    def todict(self):
        return {"sigma": self.sigma}

    @staticmethod
    def fromdict(dict):
        self = Tag()
        self.sigma = dict["sigma"]
        return self


class State(object):
    """PRF keys of the tagged file, encrypted and signed for storage on the
    server (PySwizzle.py:94-195)."""

    def __init__(self, f_key, alpha_key, chunks=0, encrypted=False, iv=None, hmac=None, key=None):
        self.f_key = f_key
        self.alpha_key = alpha_key
        self.chunks = chunks
        self.encrypted = encrypted
        self.iv = b"" if iv is None else iv
        if hmac is None and key is not None:
            self.hmac = self.get_hmac(key)
        else:
            self.hmac = hmac

    def todict(self):
        return {"f_key": hb_encode(self.f_key),
                "alpha_key": hb_encode(self.alpha_key),
                "chunks": self.chunks,
                "encrypted": self.encrypted,
                "iv": hb_encode(self.iv),
                "hmac": hb_encode(self.hmac)}

    @staticmethod
    def fromdict(dict):
        return State(hb_decode(dict["f_key"]), hb_decode(dict["alpha_key"]), dict["chunks"],
                     dict["encrypted"], hb_decode(dict["iv"]), hb_decode(dict["hmac"]))

    def get_hmac(self, key):
        """HMAC-SHA256 over iv | str(chunks) | f_key | alpha_key | str(encrypted)."""
        if isinstance(key, str):
            key = key.encode("latin-1")
        h = _hmac.new(bytes(key), None, hashlib.sha256)
        h.update(self.iv)
        h.update(str(self.chunks).encode())
        h.update(self.f_key)
        h.update(self.alpha_key)
        h.update(str(self.encrypted).encode())
        return h.digest()

    def encrypt(self, key):
        """AES-CFB8 encrypt both keys with a fresh IV, then sign."""
        if self.encrypted:
            return
        self.iv = _random_bytes(AES_BLOCK)
        nf = len(self.f_key)
        ct = _native.aes_cfb8(_kb(key), self.iv, bytes(self.f_key) + bytes(self.alpha_key), True)
        self.f_key, self.alpha_key = ct[:nf], ct[nf:]
        self.encrypted = True
        self.hmac = self.get_hmac(key)

    def decrypt(self, key):
        """Check the signature, then decrypt the keys."""
        if self.get_hmac(key) != self.hmac:
            raise HeartbeatError("Signature invalid on state.")
        if not self.encrypted:
            return
        nf = len(self.f_key)
        pt = _native.aes_cfb8(_kb(key), self.iv, bytes(self.f_key) + bytes(self.alpha_key), False)
        self.f_key, self.alpha_key = pt[:nf], pt[nf:]
        self.encrypted = False
        self.hmac = self.get_hmac(key)


_kb = _many._kb


class Proof(object):
    """Proof of storage: mu_j per sector and sigma."""

    def __init__(self):
        self.mu = list()
        self.sigma = None

    def todict(self):
        return {"mu": self.mu, "sigma": self.sigma}

    @staticmethod
    def fromdict(dict):
        self = Proof()
        self.mu = dict["mu"]
        self.sigma = dict["sigma"]
        return self


# ---------------------------------------------------------------- scheme
class PySwizzle(object):
    """Shacham-Waters private proof of storage, GPU-backed."""

    def __init__(self, sectors=10, key=None, prime=None, primebits=1024):
        self.key = _random_bytes(32) if key is None else key
        self.prime = getPrime(primebits) if prime is None else prime
        self.sectors = sectors
        self.sectorsize = self.prime.bit_length() // 8

    @staticmethod
    def generate_many(count, sectors=10, primebits=1024):
        """`count` new objects, each with its own random key and its own
        prime: the primes are drawn together on the GPU (primes.getPrimes)
        instead of one getPrime per constructor."""
        return [PySwizzle(sectors, None, p, primebits) for p in getPrimes(primebits, count)]

    def todict(self):
        return {"key": hb_encode(self.key), "prime": self.prime, "sectors": self.sectors}

    @staticmethod
    def fromdict(dict):
        return PySwizzle(dict["sectors"], hb_decode(dict["key"]), dict["prime"])

    def get_public(self):
        """A copy without the private key (a fresh random key is drawn)."""
        return PySwizzle(self.sectors, None, self.prime)

    # -- helpers
    def _check(self):
        if self.sectorsize < 1:
            raise HeartbeatError("prime must be at least 2^8 (sector size of at least one byte)")
        if int(self.sectors) < 1:
            raise HeartbeatError("sectors must be positive")

    def encode(self, file):
        """Tag every block of `file` (from its current position to EOF)."""
        self._check()
        p = int(self.prime)
        state = State(_random_bytes(32), _random_bytes(32))
        tag, nblocks = encode_file(p, int(self.sectors), state.f_key, state.alpha_key, file)
        state.chunks = nblocks
        state.encrypt(self.key)
        return (tag, state)

    def encode_many(self, files):
        """Tag every file of `files` in one batched GPU call
        (hb_encode_many): [(Tag, State), ...], each file with fresh random
        keys, exactly as a loop of encode() (PySwizzle.py:279-311) -- which
        pays every file's longest PRF rejection chain in turn."""
        self._check()
        files = list(files)
        p = int(self.prime)
        states = [State(_random_bytes(32), _random_bytes(32)) for _ in files]
        res = encode_files(p, int(self.sectors), [(s.f_key, s.alpha_key) for s in states], files)
        out = []
        for state, (tag, nblocks) in zip(states, res):
            state.chunks = nblocks
            state.encrypt(self.key)
            out.append((tag, state))
        return out

    @staticmethod
    def encode_mixed(items):
        """b.encode(file) of every (beat, file) of `items`, with any mix of
        beats -- primes, sector counts -- in one batched GPU call
        (hb_encode_mixed): a process that keeps one beat per owner, contract or
        farmer, each with its own prime (PySwizzle.py:250-251), and tags one
        file for each.  [(Tag, State), ...], exactly what
        [b.encode(f) for b, f in items] returns (PySwizzle.py:279-311 per
        item): fresh random keys per file, each state encrypted under its own
        beat's key, each file read from its current position to EOF and left
        there.  Every beat is checked before any file is read, and the
        HeartbeatError is that of the first item a loop would raise it for.  A
        batch of fewer than ENCODE_MIXED_MIN items goes through encode()."""
        items = list(items)
        for beat, _ in items:
            beat._check()
        if len(items) < ENCODE_MIXED_MIN:
            return [beat.encode(file) for beat, file in items]
        states = [State(_random_bytes(32), _random_bytes(32)) for _ in items]
        res = encode_files_mixed([(int(beat.prime), int(beat.sectors), s.f_key, s.alpha_key, file)
                                  for (beat, file), s in zip(items, states)])
        out = []
        for (beat, _), state, (tag, nblocks) in zip(items, states, res):
            state.chunks = nblocks
            state.encrypt(beat.key)
            out.append((tag, state))
        return out

    # -- re-tagging listed blocks after an edit or an append
    def _sorted_blocks(self, blocks):
        """[(index, bytes)] in ascending order of index; every index once and
        inside [0, 2^64)."""
        return _blocks.sorted_blocks(blocks, 64)

    def _open_state(self, state):
        """A decrypted copy of `state` (its signature checked); the argument
        is left as it was."""
        st = copy.copy(state)
        st.decrypt(self.key)
        return st

    def _pack_blocks(self, blocks):
        """(indices, packed bytes) of ascending blocks for one descriptor of
        hb_encode_blocks_many: all blocks whole but possibly the last."""
        return _blocks.pack_blocks(int(self.sectors) * self.sectorsize, blocks)

    def encode_blocks(self, state, blocks):
        """New tag values of listed blocks under the state's keys: `blocks` is
        an iterable of (index, bytes).  Returns (indices, Tag): the indices in
        ascending order and a Tag holding tag_i = F(i) + sum_j alpha_j m_ij mod
        p (PySwizzle.py:296-309) of each, in that order -- the patch an owner
        sends to the server (patch_tag).  Every block must be whole (sectors x
        sectorsize bytes) except the one of the highest index, which may be
        short.  The state's signature is checked and a copy is decrypted; the
        argument is left as it was."""
        self._check()
        st = self._open_state(state)
        blocks = self._sorted_blocks(blocks)
        indices, data = self._pack_blocks(blocks)
        p = int(self.prime)
        raw = encode_blocks_many(p, int(self.sectors), [(st.f_key, st.alpha_key, indices, data)])[0]
        return indices, Tag._from_raw(memoryview(raw), _native.width_of(p))

    @staticmethod
    def patch_tag(tag, indices, values, nblocks=None):
        """A new Tag of `nblocks` values (default len(tag)): those of `tag`
        with values[k] in place of block indices[k].  No key is needed: this is
        the server's side of an update.  `values` is a Tag or a sequence of
        ints.  A longer result must have every added index listed; a shorter
        one drops the rest.  A tag that holds its fixed-width image keeps one;
        a tag built from a list (fromdict) stays a list."""
        return _blocks.patch_tag(Tag, tag, indices, values, nblocks)

    def _plan_update(self, state, blocks, length):
        """What update() checks before any GPU work: (n', ascending blocks)."""
        return _blocks.plan_update(int(self.sectors) * self.sectorsize, state.chunks, blocks, length)

    def _finish_update(self, tag, st, n_new, indices, raw):
        new_tag = PySwizzle.patch_tag(tag, indices, Tag._from_raw(memoryview(raw), _native.width_of(int(self.prime))),
                                      n_new)
        new_state = State(st.f_key, st.alpha_key, n_new)
        new_state.encrypt(self.key)
        return new_tag, new_state

    def update(self, tag, state, blocks, length=None):
        """The tag and state of a file after an edit, an append or a
        truncation, from the changed blocks alone: `blocks` is an iterable of
        (index, new bytes), `length` the file's new length (None: the block
        count stays state.chunks).  With C = sectors x sectorsize and n' =
        length // C + 1: every listed block below n' - 1 must be C bytes, block
        n' - 1 must be length % C bytes (any length below C without `length`);
        an index >= n', a repeated index, or -- when n' differs from
        state.chunks -- a missing index between min(n, n') - 1 and n' - 1
        raises HeartbeatError naming the first such index, before any GPU work.
        A file that grows therefore needs its old last block, with its new
        bytes.  Returns (Tag, State): the tag with the listed values replaced
        (patch_tag), and a state of n' chunks under the same f_key and
        alpha_key, encrypted and signed with a fresh IV as encode returns it.
        Neither argument is modified."""
        self._check()
        st = self._open_state(state)
        n_new, listed = self._plan_update(st, blocks, length)
        indices, data = self._pack_blocks(listed)
        raw = encode_blocks_many(int(self.prime), int(self.sectors), [(st.f_key, st.alpha_key, indices, data)])[0]
        return self._finish_update(tag, st, n_new, indices, raw)

    def _file_blocks(self, state, fb, changed):
        """(blocks, length) of update_file: the blocks the byte ranges touch
        and those the length rule demands, read from the file's buffer."""
        return _blocks.file_blocks(int(self.sectors) * self.sectorsize, state.chunks, fb, changed)

    def update_file(self, tag, state, file, changed):
        """update() from the new file itself: `changed` is a list of (offset,
        nbytes) ranges of the NEW file that differ from the tagged one.  The
        new length is the file's; the blocks re-tagged are those the ranges
        touch plus the ones update()'s length rule demands.  The file is read
        from its start and its position is left where it was."""
        self._check()
        fb = FileBuffer(file, from_start=True)
        try:
            blocks, length = self._file_blocks(state, fb, changed)
        finally:
            fb.restore()
            fb.close()
        return self.update(tag, state, blocks, length)

    def update_many(self, items):
        """update(tag, state, blocks, length) of every item of `items` in one
        batched GPU call (hb_encode_blocks_many): [(Tag, State), ...], exactly
        what a loop of update() returns, and the HeartbeatError of the first
        item a loop would raise it for, before any GPU work.  Items whose key
        length differs from the first one's, and a batch of fewer than
        UPDATE_MANY_MIN items, go through update() one by one."""
        items = [(tag, state, list(blocks), length) for tag, state, blocks, length in items]
        self._check()
        pre = []
        for tag, state, blocks, length in items:
            st = self._open_state(state)
            n_new, listed = self._plan_update(st, blocks, length)
            indices, data = self._pack_blocks(listed)
            pre.append((st, n_new, indices, data))
        if len(items) < UPDATE_MANY_MIN:
            return [self.update(*item) for item in items]
        klen = (len(_kb(pre[0][0].f_key)), len(_kb(pre[0][0].alpha_key))) if pre else None
        batch = [k for k, t in enumerate(pre) if (len(_kb(t[0].f_key)), len(_kb(t[0].alpha_key))) == klen
                 and klen[0] == klen[1]]
        raws = encode_blocks_many(int(self.prime), int(self.sectors),
                                  [(pre[k][0].f_key, pre[k][0].alpha_key, pre[k][2], pre[k][3]) for k in batch])
        out = [None] * len(items)
        for k, raw in zip(batch, raws):
            st, n_new, indices, _ = pre[k]
            out[k] = self._finish_update(items[k][0], st, n_new, indices, raw)
        for k, item in enumerate(items):
            if out[k] is None:
                out[k] = self.update(*item)
        return out

    def gen_challenge(self, state):
        """Challenge every block once on average (chunks = #blocks, v_max = p)."""
        state.decrypt(self.key)
        return Challenge(state.chunks, self.prime, _random_bytes(32))

    def prove(self, file, chal, tag):
        """mu_j = sum v_i m_{idx_i,j} mod p, sigma = sum v_i tag[idx_i] mod p."""
        self._check()
        p = int(self.prime)
        S = int(self.sectors)
        w = _native.width_of(p)
        ntags = len(tag)
        chunks = int(chal.chunks)
        proof = Proof()
        if chunks <= 0:
            proof.mu = [0] * S
            proof.sigma = 0
            return proof
        if ntags == 0:
            raise HeartbeatError("tag is empty")
        tags_raw = tag.raw(p)
        key = _kb(chal.key)
        vmax = _native.be(int(chal.v_max))
        # absolute offsets from the start of the file, as the reference's
        # file.seek(pos) before every read (PySwizzle.py:353-355)
        fb = FileBuffer(file, from_start=True)
        try:
            tarr = np.frombuffer(tags_raw, dtype=np.uint8)
            proof.mu, proof.sigma = multi.prove_shards(p, S, key, chunks, vmax, tarr.ctypes.data, ntags,
                                                       fb.addr, fb.len, 0, multi.devices())
        finally:
            fb.restore()
            fb.close()
        return proof

    def prove_many(self, items):
        """prove() of every (file, chal, tag) of `items` in one batched GPU
        call (hb_prove_many): [Proof, ...], exactly what a loop of prove()
        (PySwizzle.py:333-370) returns -- a zero proof for chunks <= 0 -- and
        HeartbeatError("tag is empty") at the first item a loop would raise it
        for.  Every item is checked before any GPU work, so a failing item
        costs no launch.  Items whose key length differs from the batch's
        majority go through prove() one by one, and so do challenges that
        prove() would shard over several GPUs and a batch of fewer than
        PROVE_MANY_MIN items."""
        items = list(items)
        p = int(self.prime)
        S = int(self.sectors)
        out = [None] * len(items)
        cand = []
        for i, (file, chal, tag) in enumerate(items):
            self._check()
            if int(chal.chunks) <= 0:
                out[i] = Proof()
                out[i].mu = [0] * S
                out[i].sigma = 0
            elif len(tag) == 0:
                raise HeartbeatError("tag is empty")
            else:
                cand.append(i)
        ndev = len(multi.devices())
        lens = [len(_kb(items[i][1].key)) for i in cand]
        major = max(set(lens), key=lens.count) if lens else 0
        batch = [i for i, kl in zip(cand, lens) if kl == major and
                 multi.shard_count(ndev, int(items[i][1].chunks), multi.MIN_SHARD_CHUNKS) == 1]
        if len(batch) < PROVE_MANY_MIN:
            batch = []
        if batch:
            res = prove_files(p, S, [(items[i][1].key, int(items[i][1].chunks), int(items[i][1].v_max),
                                      items[i][2], items[i][0]) for i in batch])
            for i, (mu, sigma) in zip(batch, res):
                out[i] = Proof()
                out[i].mu, out[i].sigma = mu, sigma
        for i, (file, chal, tag) in enumerate(items):
            if out[i] is None:
                out[i] = self.prove(file, chal, tag)
        return out

    def verify(self, proof, chal, state):
        """True iff proof.sigma == sum v_i F(idx_i) + sum alpha_j mu_j mod p."""
        state.decrypt(self.key)
        self._check()
        p = int(self.prime)
        S = int(self.sectors)
        w = _native.width_of(p)
        chunks = int(chal.chunks)
        if chunks > 0 and int(state.chunks) <= 0:
            raise HeartbeatError("state has no chunks")
        mu = list(proof.mu)
        if len(mu) < S:
            raise HeartbeatError("proof has fewer than %d mu values" % S)
        mub = b"".join((int(m) % p).to_bytes(w, "big") for m in mu[:S])
        vmax = _native.be(int(chal.v_max)) if chunks > 0 else b"\x01"
        rhs = ctypes.create_string_buffer(w)
        ctx = multi.primary_context()
        pb = _native.be(p)
        fk, ak, ck = _kb(state.f_key), _kb(state.alpha_key), _kb(chal.key)
        with ctx.lock:
            ctx.check(_native.lib().hb_verify_rhs(ctx.h, pb, len(pb), S, fk, ak, len(fk),
                                                  int(state.chunks), ck, len(ck), max(chunks, 0),
                                                  vmax, len(vmax), mub, rhs))
        return proof.sigma == int.from_bytes(rhs.raw, "big")

    def verify_many(self, items):
        """verify() of every (proof, chal, state) of `items` in one batched
        GPU call (hb_verify_rhs_many): [bool, ...], exactly what a loop of
        verify() (PySwizzle.py:372-395) returns, and the same HeartbeatError
        at the first item a loop would raise it for (bad signature, too few
        mu values, a state without chunks).  Every item is checked before any
        GPU work, so a failing item costs no launch.  Items whose key lengths
        differ from the batch's majority go through verify() one by one, and
        so does a batch of fewer than VERIFY_MANY_MIN items."""
        items = list(items)
        p = int(self.prime)
        S = int(self.sectors)
        pre = []
        for proof, chal, state in items:
            state.decrypt(self.key)
            self._check()
            chunks = int(chal.chunks)
            if chunks > 0 and int(state.chunks) <= 0:
                raise HeartbeatError("state has no chunks")
            mu = list(proof.mu)
            if len(mu) < S:
                raise HeartbeatError("proof has fewer than %d mu values" % S)
            pre.append((_kb(state.f_key), _kb(state.alpha_key), int(state.chunks), _kb(chal.key),
                        max(chunks, 0), int(chal.v_max) if chunks > 0 else 1, mu[:S]))
        if not pre:
            return []
        lens = [(len(t[0]), len(t[1]), len(t[3])) for t in pre]
        major = max(set(lens), key=lens.count)
        batch = [i for i, kl in enumerate(lens) if kl == major and kl[0] == kl[1]]
        if len(batch) < VERIFY_MANY_MIN:
            batch = []
        out = [None] * len(items)
        if batch:
            rhs = verify_rhs_many(p, S, [pre[i] for i in batch])
            for i, r in zip(batch, rhs):
                out[i] = items[i][0].sigma == r
        for i, (proof, chal, state) in enumerate(items):
            if out[i] is None:
                out[i] = self.verify(proof, chal, state)
        return out

    @staticmethod
    def prove_mixed(items):
        """b.prove(file, chal, tag) of every (beat, file, chal, tag) of
        `items`, with any mix of beats -- primes, sector counts, challenge key
        lengths -- in one batched GPU call (hb_prove_mixed): the proofs a
        storage node owes to many owners, each of whom drew their own prime
        (PySwizzle.py:250-251).  [Proof, ...], exactly what
        [b.prove(f, c, t) for b, f, c, t in items] returns (PySwizzle.py:333-370
        per item) -- a zero proof for chunks <= 0 -- and the same
        HeartbeatError at the first item a loop would raise it for.  Every
        item is checked before any GPU work.  Challenges that prove() would
        shard over several GPUs go through prove(), and so does a batch of
        fewer than PROVE_MANY_MIN items."""
        items = list(items)
        out = [None] * len(items)
        cand = []
        for i, (beat, file, chal, tag) in enumerate(items):
            beat._check()
            if int(chal.chunks) <= 0:
                out[i] = Proof()
                out[i].mu = [0] * int(beat.sectors)
                out[i].sigma = 0
            elif len(tag) == 0:
                raise HeartbeatError("tag is empty")
            else:
                cand.append(i)
        ndev = len(multi.devices())
        batch = [i for i in cand
                 if multi.shard_count(ndev, int(items[i][2].chunks), multi.MIN_SHARD_CHUNKS) == 1]
        if len(batch) < PROVE_MANY_MIN:
            batch = []
        if batch:
            res = _many.prove_files_mixed(
                [(int(items[i][0].prime), int(items[i][0].sectors), items[i][2].key, int(items[i][2].chunks),
                  int(items[i][2].v_max), items[i][3], items[i][1]) for i in batch])
            for i, (mu, sigma) in zip(batch, res):
                out[i] = Proof()
                out[i].mu, out[i].sigma = mu, sigma
        for i, (beat, file, chal, tag) in enumerate(items):
            if out[i] is None:
                out[i] = beat.prove(file, chal, tag)
        return out

    @staticmethod
    def verify_mixed(items):
        """b.verify(proof, chal, state) of every (beat, proof, chal, state) of
        `items`, with any mix of beats, in one batched GPU call
        (hb_verify_rhs_mixed): an auditor checking the proofs of several
        owners.  Each state is decrypted with its own beat's key.  [bool, ...],
        exactly what a loop of verify() (PySwizzle.py:372-395) returns, and
        the same HeartbeatError at the first item a loop would raise it for
        (bad signature, too few mu values, a state without chunks).  Every
        item is checked before any GPU work.  A batch of fewer than
        VERIFY_MANY_MIN items goes through verify()."""
        items = list(items)
        pre = []
        for beat, proof, chal, state in items:
            state.decrypt(beat.key)
            beat._check()
            S = int(beat.sectors)
            chunks = int(chal.chunks)
            if chunks > 0 and int(state.chunks) <= 0:
                raise HeartbeatError("state has no chunks")
            mu = list(proof.mu)
            if len(mu) < S:
                raise HeartbeatError("proof has fewer than %d mu values" % S)
            pre.append((int(beat.prime), S, _kb(state.f_key), _kb(state.alpha_key), int(state.chunks), _kb(chal.key),
                        max(chunks, 0), int(chal.v_max) if chunks > 0 else 1, mu[:S]))
        batch = [i for i, t in enumerate(pre) if len(t[2]) == len(t[3])]
        if len(batch) < VERIFY_MANY_MIN:
            batch = []
        out = [None] * len(items)
        if batch:
            rhs = _many.verify_rhs_mixed([pre[i] for i in batch])
            for i, r in zip(batch, rhs):
                out[i] = items[i][1].sigma == r
        for i, (beat, proof, chal, state) in enumerate(items):
            if out[i] is None:
                out[i] = beat.verify(proof, chal, state)
        return out

    @staticmethod
    def tag_type():
        return Tag

    @staticmethod
    def state_type():
        return State

    @staticmethod
    def challenge_type():
        return Challenge

    @staticmethod
    def proof_type():
        return Proof


# Host buffers whose bytes hb_encode page-locks read-only in windows
# (HB_HOST_REGISTER) instead of staging them through the runtime's pageable
# copies, by FileBuffer kind: all of them.  A 4 GiB real file through
# encode_file: 38.2 vs 31.1 GiB/s (registered vs pageable, best of 3), a
# BytesIO 47.7 vs 43.1, one box (profiles/r05/f/bench_c3_nocpu.log; the
# caller-pinned raw rate 48.9); the medians of 5 in a standalone probe 40.7 vs
# 30.4 for the file (profiles/r05/f/probe2.log).  bench.py's host_path
# measures both ways in every default run.
REGISTER_KINDS = ("mmap", "bytesio", "bytes", "read")
# hb_encode page-locks only host buffers of at least this many bytes (below
# it the windows cost more than they save, hb_runtime.cpp); a smaller mapped
# file is prefaulted instead (MAP_POPULATE), as without registration
HOST_REGISTER_MIN = 32 << 20


def encode_file(p, sectors, f_key, alpha_key, file, devices=None, register=None):
    """GPU encode of a file object / buffer: (Tag, number of blocks).  Files of
    at least 2 x multi.MIN_SHARD_BYTES are sharded by block range over
    `devices` (default: multi.devices(), every visible GPU).  `register`
    forces (True) or forbids (False) the windowed read-only page-locking of
    the host bytes (HB_HOST_REGISTER); None: REGISTER_KINDS decides."""
    w = _native.width_of(p)
    ss = p.bit_length() // 8
    C = ss * sectors
    fk, ak = _kb(f_key), _kb(alpha_key)
    if len(fk) != len(ak):
        raise HeartbeatError("f_key and alpha_key must have the same length")
    if register is False or (register is None and "mmap" not in REGISTER_KINDS):
        populate = True
    else:
        populate = HOST_REGISTER_MIN
    fb = FileBuffer(file, populate=populate)
    try:
        nblocks = fb.len // C + 1
        # the tags land in the array the Tag keeps: no zero fill, no copy of
        # the image (a bytes-like buffer to Tag)
        out = np.empty(nblocks * w, dtype=np.uint8)
        reg = fb.kind in REGISTER_KINDS if register is None else bool(register)
        multi.encode_shards(p, sectors, fk, ak, fb.addr, fb.len, nblocks, out.ctypes.data,
                            _native.HB_HOST_REGISTER if reg else 0, multi.devices(devices))
        fb.consume()
    finally:
        fb.close()
    return Tag._from_raw(memoryview(out), w), nblocks


def encode_files(p, sectors, keys, files):
    """Batched GPU encode (hb_encode_many) of many file objects / buffers,
    file i under keys[i] = (f_key, alpha_key): [(Tag, number of blocks), ...].
    Each file is read from its current position to EOF and left there, as by
    encode_file; all keys of a batch have one length.  Runs on
    multi.primary_context() (a batch is not spread over several GPUs)."""
    # a file is opened as its descriptor is filled
    return _many.encode_files("hb_encode_many", Tag, p, sectors, keys, files, open_first=False)


# Fewest files PySwizzle.encode_mixed sends through hb_encode_mixed; below it
# the items go through encode() one by one: the smallest file count at which
# the mixed call's slowest round beats the loop's fastest, device-resident and
# from host memory.  One file through the group's three launches only ties
# with the single encode when the bytes are on the device (1024-bit, S = 10,
# 1 MiB: 0.82-0.84 against 0.83-0.86 ms; from host memory 0.90-0.97 against
# 0.98-1.07), two files win in both (0.81-0.95 against 1.39-1.48 ms;
# 0.90-1.03 against 1.62-1.72), three by 2.6x: the --files 1, 2 and 3 rows of
# scripts/encode_mixed_rate.py, profiles/many/encode_mixed_rate.json,
# DESIGN.md 5.3i.
ENCODE_MIXED_MIN = 2


def encode_files_mixed(items):
    """Batched GPU encode (hb_encode_mixed) of the files of many owners:
    `items` is a list of (p, sectors, f_key, alpha_key, file), every file under
    its own prime, sector count and key length; returns
    [(Tag, number of blocks), ...], what encode_file gives per item.  Each file
    is read from its current position to EOF and left there.  Runs on
    multi.primary_context() (a batch is not spread over several GPUs)."""
    return _many.encode_files_mixed(items, "hb_encode_mixed", Tag, open_first=False)


# Fewest items PySwizzle.update_many sends through hb_encode_blocks_many; below
# it the items go through update() one by one: the smallest item count at
# which the batch's slowest round beats the loop's fastest, device-resident and
# from host memory (the rule of ENCODE_MIXED_MIN).  One item is the same call
# either way (1024-bit, S = 10, 4 blocks per file: 0.63-0.66 against 0.63-0.66
# ms from host memory, 0.63-0.65 against 0.62-0.64 on the device); two items
# win in both (0.64-0.67 against 1.19-1.21 ms; 0.63-0.67 against 1.17-1.21),
# three by 2.5x, 256 by 90x (1.28-1.37 against 123.6-123.8 ms): the many rows
# of scripts/blocks_rate.py, profiles/many/blocks_rate.json, DESIGN.md 5.3k.
UPDATE_MANY_MIN = 2


def encode_blocks_many(p, sectors, items):
    """Batched GPU tags of listed blocks (hb_encode_blocks_many): `items` is a
    list of (f_key, alpha_key, indices, data) with each file's listed blocks
    back to back in `data`; returns one uint8 array of tag images per item.
    Runs on multi.primary_context()."""
    return _many.encode_blocks_many(p, sectors, items)


# Fewest proofs PySwizzle.prove_many sends through hb_prove_many; below it the
# items go through prove() one by one.  One proof through the batch's three
# launches only ties with the single fused launch (1024-bit, S = 10, 820
# chunks of a 1 MiB host file: 0.81-0.85 against 0.82-0.86 ms), two proofs
# already win (1.01-1.10 against 1.80-1.84 ms), three by 2.3x:
# scripts/prove_many_rate.py, profiles/many/prove_many_rate.json, DESIGN.md 5.3c.
PROVE_MANY_MIN = 2


def prove_files(p, sectors, items):
    """Batched GPU prove (hb_prove_many) of many challenges: `items` is a list
    of (chal_key, chunks, v_max, tag, file) with a Tag and a file object /
    buffer each; returns [(mu list, sigma), ...], what hb_prove gives per item
    (PySwizzle.py:333-370).  Every file is read whole, from its start, and its
    position is left where it was, as by PySwizzle.prove.  All challenge keys
    of a batch have one length.  Runs on multi.primary_context() (a batch is
    not spread over several GPUs)."""
    return _many.prove_files("hb_prove_many", p, sectors, items)


# Fewest proofs PySwizzle.verify_many sends through hb_verify_rhs_many; below
# it the items go through verify() one by one.  One proof through the batch's
# two launches loses to the fused single launch (1024-bit, S = 10, 820 chunks:
# 1.07-1.10 against 0.90-0.94 ms; 256-bit, 129 chunks: 0.149-0.154 against
# 0.096-0.098), two proofs already win (1.08-1.15 against 1.92-1.99 ms;
# 0.150-0.172 against 0.193-0.196): scripts/verify_many_rate.py,
# profiles/many/verify_many_rate.json, DESIGN.md 5.3b.
VERIFY_MANY_MIN = 2


def verify_rhs_many(p, sectors, items):
    """Batched right-hand sides (hb_verify_rhs_many) of many proofs: `items`
    is a list of (f_key, alpha_key, state_chunks, chal_key, chunks, v_max,
    mu_list) with decrypted state keys; returns the list of ints that
    hb_verify_rhs gives per item (PySwizzle.py:381-394).  All f_keys and
    alpha_keys of a batch have one length, all challenge keys one length.  Runs
    on multi.primary_context() (a batch is not spread over several GPUs)."""
    # more than `sectors` mu values are accepted: the first `sectors` count
    return _many.verify_rhs_many("hb_verify_rhs_many", p, sectors, items, exact_mu=False)


# The reference's module path (heartbeat/PySwizzle/PySwizzle.py): pickles of
# these objects name heartbeat.PySwizzle.PySwizzle, which the repo's
# heartbeat/ package re-exports them from, so they load under either package.
for _c in (Challenge, Tag, State, Proof, PySwizzle):
    _c.__module__ = "heartbeat.PySwizzle.PySwizzle"
del _c
