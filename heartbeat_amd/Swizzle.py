"""The cxx extension's Swizzle scheme (``heartbeat.Swizzle``), GPU-backed.

Mirrors the Python surface of the PyCXX module cxx/Swizzle.hxx:43-762 over the
HIP kernels' cxx mode (``HB_PRF_CXX``): the cxx prf (cxx/prf.hxx:97-176,
CFB-128 over SHA256(LE32 i), at most 81 tries) in encode
(shacham_waters_private.cxx:638-702), prove (:731-789, check_all and unsigned
int sector offsets) and verify (:791-842).  Tags differ from PySwizzle's for
equal keys.

Object surface (Swizzle.hxx:63-311): every type -- ``Swizzle``, ``Tag``,
``State``, ``Challenge``, ``Proof`` -- is constructible without arguments and
has ``__getstate__`` (its binary serialization), ``__setstate__(state)``,
``__reduce__`` (pickle), ``todict()`` (base64 TEXT of the binary form),
static ``fromdict(text)`` and equality by serialized bytes; the ordering
comparisons raise NotImplementedError.  ``State`` adds
``encrypt(k_enc, k_mac[, convergent])``, ``decrypt(k_enc, k_mac)`` and
``keysize()`` (Swizzle.hxx:335-432).  Errors are HeartbeatError with the
reference's messages.

Binary formats follow shacham_waters_private.cxx:38-594, 844-976: u32 fields
written as ``PutWord32(htonl(x))`` and integers as ``u32 MinEncodedSize`` +
big-endian bytes.  With Crypto++'s default big-endian PutWord32 the double swap
makes every u32 LITTLE-endian on x86; that byte order, and the
formats as a whole, are parity unpinned -- Crypto++ is absent here and no
reference test pins the bytes.  The State's raw form is
``[sig_len][n, iv_len, iv, enc_len, AES-256-CFB128(k_enc, iv,
[f_key_len, f_key, alpha_key_len, alpha_key])][mac_len][HMAC-SHA256(k_mac,
signed part)]`` (:169-306).
"""
import base64
import binascii
import ctypes
import hashlib
import hmac as _hmac
import struct

import numpy as np

from . import _blocks, _many, _native, multi
from ._filebuf import FileBuffer
from .exc import HeartbeatError
from .PySwizzle.PySwizzle import _kb, _random_bytes, getPrime
from .primes import getPrimes

__all__ = ["Swizzle", "Tag", "State", "Challenge", "Proof"]

# shacham_waters_private.hxx:193 / Swizzle.hxx:494-508: the Python API fixes a
# 1024-bit prime (Crypto++ draws it below 2^1024; here exactly 1024 bits)
PRIME_BITS = 1024
KEY_SIZE = 32            # shacham_waters_private_data::key_size
MAX_RAW_SIZE = 2048      # state::max_raw_size
_FLAG_PUBLIC = 0x01


# ---------------------------------------------------------------- wire helpers
def _u32(x):
    return struct.pack("<I", int(x) & 0xffffffff)


def _min_encoded(x):
    """Crypto++ Integer::Encode(bt, MinEncodedSize()): unsigned big-endian,
    at least one byte, after its u32 length."""
    x = int(x)
    n = max(1, (x.bit_length() + 7) // 8)
    return _u32(n) + x.to_bytes(n, "big")


class _Reader(object):
    def __init__(self, data):
        self.b = bytes(data)
        self.i = 0

    def u32(self, err):
        if self.i + 4 > len(self.b):
            raise HeartbeatError(err)
        v = struct.unpack_from("<I", self.b, self.i)[0]
        self.i += 4
        return v

    def take(self, n, err):
        if self.i + n > len(self.b):
            raise HeartbeatError(err)
        v = self.b[self.i:self.i + n]
        self.i += n
        return v

    def integer(self, err):
        n = self.u32(err)
        # safe_integer (shacham_waters_private.hxx:58-75): the stream must hold n bytes
        return int.from_bytes(self.take(n, "Unable to decode integer."), "big")


class _Serializable(object):
    """PyBytesStateAccessiblePyClass (Swizzle.hxx:125-311)."""

    def _serialize(self):
        raise NotImplementedError

    def _deserialize(self, data):
        raise NotImplementedError

    def __getstate__(self):
        return self._serialize()

    def __setstate__(self, *args):
        if len(args) != 1:
            raise HeartbeatError("__setstate__ only takes one argument: state")
        try:
            self._deserialize(bytes(args[0]))
        except HeartbeatError:
            raise
        except Exception as e:   # noqa: BLE001 -- the reference maps std::exception
            raise HeartbeatError(str(e))

    def __reduce__(self):
        return (type(self), (), self.__getstate__())

    def todict(self):
        return base64.b64encode(self._serialize()).decode("utf-8")

    @classmethod
    def fromdict(cls, text):
        obj = cls()
        try:
            raw = base64.b64decode(text.encode("utf-8") if isinstance(text, str) else bytes(text))
        except (binascii.Error, ValueError, AttributeError, TypeError) as e:
            raise HeartbeatError(str(e))
        obj.__setstate__(raw)
        return obj

    def __eq__(self, other):
        if type(other) is not type(self):
            return False
        return self._serialize() == other._serialize()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __lt__(self, other):
        raise NotImplementedError("Less than operator is not implemented.")

    def __le__(self, other):
        raise NotImplementedError("Less than or equal to operator is not implemented.")

    def __gt__(self, other):
        raise NotImplementedError("Greater than operator is not implemented.")

    def __ge__(self, other):
        raise NotImplementedError("Greater than or equal to operator is not implemented.")


# ---------------------------------------------------------------- data types
class Tag(_Serializable):
    """File tag: one sigma per block (tag::serialize :38-54)."""

    def __init__(self):
        self._sigma = []
        self._raw = None
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
        t._sigma = sigma
        return t

    @property
    def sigma(self):
        if self._sigma is None:
            w, raw = self._width, bytes(self._raw)
            self._sigma = [int.from_bytes(raw[i:i + w], "big") for i in range(0, len(raw), w)]
        return self._sigma

    def __len__(self):
        if self._sigma is None:
            return len(self._raw) // self._width
        return len(self._sigma)

    def raw(self, p):
        """Fixed-width big-endian image (the GPU prove's input)."""
        w = _native.width_of(p)
        if self._raw is not None and self._width == w and self._sigma is None:
            return self._raw
        top = 1 << (8 * w)
        return b"".join((s if 0 <= s < top else s % p).to_bytes(w, "big") for s in self.sigma)

    def _serialize(self):
        out = [_u32(len(self))]
        if self._sigma is None:
            w, raw = self._width, self._raw
            for i in range(0, len(raw), w):
                v = bytes(raw[i:i + w]).lstrip(b"\0") or b"\0"
                out.append(_u32(len(v)) + v)
        else:
            out.extend(_min_encoded(s) for s in self._sigma)
        return b"".join(out)

    def _deserialize(self, data):
        r = _Reader(data)
        n = r.u32("Unable to get sigma count.")
        sig = [r.integer("Unable to get sigma size.") for _ in range(n)]
        self._sigma, self._raw, self._width = sig, None, 0


class State(_Serializable):
    """Encrypted and signed file state: n (blocks), f_key, alpha_key
    (state, shacham_waters_private.cxx:80-458)."""

    def __init__(self):
        self.n = 0
        self.f_key = b""
        self.alpha_key = b""
        self._raw = None
        self.encrypted = False

    @property
    def chunks(self):
        return self.n

    def keysize(self):
        return KEY_SIZE

    @staticmethod
    def _key(k):
        try:
            k = _kb(k)
        except (TypeError, AttributeError, UnicodeEncodeError):
            raise HeartbeatError("Invalid encryption key.")
        if len(k) != KEY_SIZE:
            raise HeartbeatError("Encryption key must be %d bytes in length.  Use keysize() to retrieve "
                                 "the key size." % KEY_SIZE)
        return k

    def encrypt(self, *args):
        """encrypt(k_enc, k_mac[, convergent]) -- encrypt_and_sign (:169-306);
        convergent encryption uses a zero IV."""
        if len(args) < 2:
            raise HeartbeatError("encrypt() takes at least two arguments: the encryption key and the mac key "
                                 "and an optional argument a bool, whether to use convergent encryption")
        k_enc, k_mac = self._key(args[0]), self._key(args[1])
        convergent = len(args) > 2 and bool(args[2])
        iv = b"\0" * 16 if convergent else _random_bytes(16)
        plain = _u32(len(self.f_key)) + bytes(self.f_key) + _u32(len(self.alpha_key)) + bytes(self.alpha_key)
        enc = _native.aes_cfb128(k_enc, iv, plain, True)
        sig = _u32(self.n) + _u32(len(iv)) + iv + _u32(len(enc)) + enc
        mac = _hmac.new(k_mac, sig, hashlib.sha256).digest()
        self._raw = _u32(len(sig)) + sig + _u32(len(mac)) + mac
        self.encrypted = True

    def _check_sig_and_decrypt(self, k_enc, k_mac):
        """check_sig_and_decrypt (:308-438): False on a bad signature."""
        if not self.encrypted:
            raise HeartbeatError("in shacham_waters_private_data::state::check_sig_and_decrypt, data must be "
                                 "encrypted before decryption and checking signature.")
        r = _Reader(self._raw)
        sig = r.take(r.u32("Unable to get signed data size."), "Incorrect size transferred.")
        msz = r.u32("Unable to get mac size.")
        if msz != 32:
            return False
        mac = r.take(msz, "Incorrect size transferred.")
        if not _hmac.compare_digest(_hmac.new(k_mac, sig, hashlib.sha256).digest(), mac):
            return False
        s = _Reader(sig)
        self.n = s.u32("Unable to get n.")
        iv = s.take(s.u32("Unable to get iv size."), "Unable to get iv.")
        enc = s.take(s.u32("Unable to get encrypted size."), "Unable to get encrypted data.")
        plain = _native.aes_cfb128(k_enc, iv, enc, False)
        p = _Reader(plain)
        self.f_key = p.take(p.u32("Unable to get key size."), "Key corrupted.")
        self.alpha_key = p.take(p.u32("Unable to get key size."), "Key corrupted.")
        return True

    def decrypt(self, *args):
        """decrypt(k_enc, k_mac): restores the keys on success; a bad
        signature leaves the state as it is (Swizzle.hxx:383-406 ignores the
        result of check_sig_and_decrypt)."""
        if len(args) != 2:
            raise HeartbeatError("decrypt() takes two arguments: the encryption key and the mac key.")
        self._check_sig_and_decrypt(self._key(args[0]), self._key(args[1]))

    def _serialize(self):
        if not self.encrypted:
            raise HeartbeatError("in shacham_waters_private_data::serialize, state must be encrypted prior "
                                 "to serialization.")
        return _u32(len(self._raw)) + self._raw

    def _deserialize(self, data):
        r = _Reader(data)
        n = r.u32("Unable to get raw size of state.")
        if n > MAX_RAW_SIZE:
            raise HeartbeatError("Reported size of encrypted state is too large.")
        self._raw = r.take(n, "Raw data incorrect size.")
        self.encrypted = True
        # public_interpretation (:440-458): n is readable without the keys
        pr = _Reader(self._raw)
        pr.u32("Unable to get n.")
        self.n = pr.u32("Unable to get n.")
        self.f_key = b""
        self.alpha_key = b""

    def _copy(self):
        s = State()
        s.n, s.f_key, s.alpha_key = self.n, self.f_key, self.alpha_key
        s._raw, s.encrypted = self._raw, self.encrypted
        return s


class Challenge(_Serializable):
    """l (indices to check), key, v_max (challenge :460-525)."""

    def __init__(self, chunks=0, v_max=0, key=b""):
        self.chunks = chunks
        self.v_max = v_max
        self.key = key

    def _serialize(self):
        k = bytes(self.key)
        return _u32(self.chunks) + _u32(len(k)) + k + _min_encoded(self.v_max)

    def _deserialize(self, data):
        r = _Reader(data)
        self.chunks = r.u32("Unable to read l.")
        ks = r.u32("Unable to read key size.")
        if ks > KEY_SIZE:
            raise HeartbeatError("Invalid key size.")
        self.key = r.take(ks, "Key corrupted.")
        self.v_max = r.integer("Unable to read B size.")


class Proof(_Serializable):
    """mu_j and sigma (proof :527-594)."""

    def __init__(self):
        self.mu = []
        self.sigma = 0

    def _serialize(self):
        return _u32(len(self.mu)) + b"".join(_min_encoded(m) for m in self.mu) + _min_encoded(self.sigma)

    def _deserialize(self, data):
        r = _Reader(data)
        n = r.u32("Unable to retrieve proof mu count.")
        self.mu = [r.integer("Unable to retrieve integer size.") for _ in range(n)]
        self.sigma = r.integer("Unable to read sigma size.")


# ---------------------------------------------------------------- scheme
class Swizzle(_Serializable):
    """Shacham-Waters private proof of storage with the cxx extension's prf
    (shacham_waters_private.hxx:125-229; Python type Swizzle.hxx:475-735).
    Serialization keeps the reference's fields (flags, keys unless public,
    sectors, sector size, p; :844-976): check_fraction is not part of it, so a
    deserialized object has the constructor default 1.0, as in the reference."""

    def __init__(self, check_fraction=1.0, sectors=10, initialize=True, prime=None):
        self.check_fraction = float(check_fraction)
        self.sectors = int(sectors)
        self.public = False
        self.k_enc = b"\0" * KEY_SIZE
        self.k_mac = b"\0" * KEY_SIZE
        self.prime = 0 if prime is None else int(prime)
        if initialize:
            # init (:596-624): random keys, a random prime, sector size BitCount/8
            self.k_enc = _random_bytes(KEY_SIZE)
            self.k_mac = _random_bytes(KEY_SIZE)
            if prime is None:
                self.prime = getPrime(PRIME_BITS)
        self.sectorsize = self.prime.bit_length() // 8   # _p.BitCount()/8 (:621)

    @classmethod
    def generate_many(cls, count, check_fraction=1.0, sectors=10):
        """`count` new objects, each with its own random keys and its own
        prime: the primes are drawn together on the GPU (primes.getPrimes)
        instead of one getPrime per constructor."""
        return [cls(check_fraction, sectors, True, p) for p in getPrimes(PRIME_BITS, count)]

    # -- serialisation (:844-976)
    def __reduce__(self):
        # the reference reduces to (type, (), state): a default-constructed
        # object whose fields __setstate__ then replaces; constructing it
        # uninitialized skips drawing a prime that is thrown away
        return (Swizzle, (1.0, 10, False), self.__getstate__())

    @classmethod
    def fromdict(cls, text):
        obj = cls(initialize=False)
        try:
            raw = base64.b64decode(text.encode("utf-8") if isinstance(text, str) else bytes(text))
        except (binascii.Error, ValueError, AttributeError, TypeError) as e:
            raise HeartbeatError(str(e))
        obj.__setstate__(raw)
        return obj

    def _serialize(self):
        out = [bytes([_FLAG_PUBLIC if self.public else 0])]
        if not self.public:
            out += [_u32(KEY_SIZE), bytes(self.k_enc), _u32(KEY_SIZE), bytes(self.k_mac)]
        out += [_u32(self.sectors), _u32(self.sectorsize), _min_encoded(self.prime)]
        return b"".join(out)

    def _deserialize(self, data):
        r = _Reader(data)
        f = r.take(1, "Unable to retrieve heartbeat flags.")[0]
        self.public = bool(f & _FLAG_PUBLIC)
        if not self.public:
            for attr in ("k_enc", "k_mac"):
                if r.u32("Unable to retrieve key size.") != KEY_SIZE:
                    raise HeartbeatError("Incompatible key sizes.")
                setattr(self, attr, r.take(KEY_SIZE, "Key corrupted."))
        self.sectors = r.u32("Unable to read sector count.")
        self.sectorsize = r.u32("Unable to read sector size.")
        self.prime = r.integer("Unable to read p size.")

    def get_public(self):
        """A copy with the keys zeroed (get_public, :626-636)."""
        s = Swizzle(self.check_fraction, self.sectors, initialize=False, prime=self.prime)
        s.sectorsize = self.sectorsize
        s.public = True
        return s

    def _check(self):
        if self.sectorsize < 1:
            raise HeartbeatError("prime must be at least 2^8 (sector size of at least one byte)")
        if self.sectors < 1:
            raise HeartbeatError("sectors must be positive")

    # -- scheme
    def encode(self, file):
        """(Tag, State) of every block of `file` from its position to EOF
        (encode :638-702); the state is encrypted and signed."""
        self._check()
        p = self.prime
        w = _native.width_of(p)
        C = self.sectorsize * self.sectors
        state = State()
        state.f_key = _random_bytes(KEY_SIZE)
        state.alpha_key = _random_bytes(KEY_SIZE)
        fb = FileBuffer(file)
        try:
            nblocks = fb.len // C + 1
            out = np.empty(nblocks * w, dtype=np.uint8)
            multi.encode_shards(p, self.sectors, state.f_key, state.alpha_key, fb.addr, fb.len, nblocks,
                                out.ctypes.data, _native.HB_PRF_CXX, multi.devices())
            fb.consume()
        finally:
            fb.close()
        state.n = nblocks
        state.encrypt(self.k_enc, self.k_mac)
        return Tag._from_raw(memoryview(out), w), state

    def encode_many(self, files):
        """[(Tag, State), ...] of every file of `files` in one batched GPU
        call (hb_cxx_encode_many): exactly what a loop of encode() returns --
        fresh keys per file, each state encrypted and signed, each file read
        from its position to EOF and left there.  Fewer than
        CXX_ENCODE_MANY_MIN files go through encode() one by one."""
        self._check()
        files = list(files)
        if len(files) < CXX_ENCODE_MANY_MIN:
            return [self.encode(f) for f in files]
        states = []
        for _ in files:
            state = State()
            state.f_key = _random_bytes(KEY_SIZE)
            state.alpha_key = _random_bytes(KEY_SIZE)
            states.append(state)
        res = encode_files(self.prime, self.sectors, [(s.f_key, s.alpha_key) for s in states], files)
        out = []
        for state, (tag, nblocks) in zip(states, res):
            state.n = nblocks
            state.encrypt(self.k_enc, self.k_mac)
            out.append((tag, state))
        return out

    @staticmethod
    def encode_mixed(items):
        """b.encode(file) of every (beat, file) of `items`, with any mix of
        beats -- primes, sector counts -- in one batched GPU call
        (hb_cxx_encode_mixed): a process that keeps one beat per owner, each
        with its own prime (init, shacham_waters_private.cxx:596-624), and tags
        one file for each.  [(Tag, State), ...], exactly what
        [b.encode(f) for b, f in items] returns (:638-702 per item): fresh keys
        per file, each state encrypted and signed under its own beat's keys,
        each file read from its position to EOF and left there.  Every beat is
        checked before any file is read, and the HeartbeatError is that of the
        first item a loop would raise it for.  A batch of fewer than
        CXX_ENCODE_MIXED_MIN items goes through encode()."""
        items = list(items)
        for beat, _ in items:
            beat._check()
        if len(items) < CXX_ENCODE_MIXED_MIN:
            return [beat.encode(file) for beat, file in items]
        states = []
        for _ in items:
            state = State()
            state.f_key = _random_bytes(KEY_SIZE)
            state.alpha_key = _random_bytes(KEY_SIZE)
            states.append(state)
        res = encode_files_mixed([(beat.prime, beat.sectors, s.f_key, s.alpha_key, file)
                                  for (beat, file), s in zip(items, states)])
        out = []
        for (beat, _), state, (tag, nblocks) in zip(items, states, res):
            state.n = nblocks
            state.encrypt(beat.k_enc, beat.k_mac)
            out.append((tag, state))
        return out

    # -- re-tagging listed blocks after an edit or an append
    def _open_state(self, state):
        """A decrypted copy of `state`; the argument is left as it was.  A bad
        signature raises: the reference's decrypt ignores it (Swizzle.hxx:383-406),
        but tags made under garbage keys would corrupt a tag silently."""
        s = state._copy()
        if not s._check_sig_and_decrypt(self.k_enc, self.k_mac):
            raise HeartbeatError("Signature check or decryption failed in updating tags.  "
                                 "State of remote file cannot be verified.")
        return s

    def _block_bytes(self):
        return int(self.sectors) * int(self.sectorsize)

    def encode_blocks(self, state, blocks):
        """New tag values of listed blocks under the state's keys: `blocks` is
        an iterable of (index, bytes).  Returns (indices, Tag): the indices in
        ascending order and a Tag holding each block's sigma
        (shacham_waters_private.cxx:674-694 for chunk_id = index), in that
        order -- the patch an owner sends to the server (patch_tag).  Every
        block must be whole (sectors x sectorsize bytes) except the one of the
        highest index, which may be short; an empty one keeps f(index)
        unreduced (:681-690).  An index is the prf's unsigned int: below 2^32.
        The state's signature is checked and a copy is decrypted; the argument
        is left as it was."""
        self._check()
        st = self._open_state(state)
        indices, data = _blocks.pack_blocks(self._block_bytes(), _blocks.sorted_blocks(blocks, 32))
        raw = encode_blocks_many(self.prime, self.sectors, [(st.f_key, st.alpha_key, indices, data)])[0]
        return indices, Tag._from_raw(memoryview(raw), _native.width_of(self.prime))

    @staticmethod
    def patch_tag(tag, indices, values, nblocks=None):
        """A new Tag of `nblocks` values (default len(tag)): those of `tag`
        with values[k] in place of block indices[k].  No key is needed: this is
        the server's side of an update.  `values` is a Tag or a sequence of
        ints.  A longer result must have every added index listed; a shorter
        one drops the rest.  A tag that holds its fixed-width image keeps one
        (one numpy copy); a tag built from a list (fromdict) stays a list."""
        return _blocks.patch_tag(Tag, tag, indices, values, nblocks)

    def _plan_update(self, st, blocks, length):
        """What update() checks before any GPU work, on the opened state:
        (n', indices, packed bytes)."""
        C = self._block_bytes()
        if length is not None and int(length) // C + 1 >= 1 << 32:
            raise HeartbeatError("a file of %d blocks does not fit the state's 32-bit block count"
                                 % (int(length) // C + 1))
        n_new, listed = _blocks.plan_update(C, st.n, blocks, length)
        indices, data = _blocks.pack_blocks(C, listed)
        return n_new, indices, data

    def _finish_update(self, tag, st, n_new, indices, raw):
        new_tag = Swizzle.patch_tag(tag, indices, Tag._from_raw(memoryview(raw), _native.width_of(self.prime)), n_new)
        new_state = State()
        new_state.n, new_state.f_key, new_state.alpha_key = n_new, st.f_key, st.alpha_key
        new_state.encrypt(self.k_enc, self.k_mac)
        return new_tag, new_state

    def update(self, tag, state, blocks, length=None):
        """The tag and state of a file after an edit, an append or a
        truncation, from the changed blocks alone: `blocks` is an iterable of
        (index, new bytes), `length` the file's new length (None: the block
        count stays state.n).  With C = sectors x sectorsize and n' =
        length // C + 1: every listed block below n' - 1 must be C bytes, block
        n' - 1 must be length % C bytes (any length below C without `length`);
        an index >= n', a repeated index, or -- when n' differs from state.n --
        a missing index between min(n, n') - 1 and n' - 1 raises
        HeartbeatError naming the first such index, and so do a state whose
        signature does not check and n' >= 2^32 (the state's n is a u32), all
        before any GPU work.  A file that grows therefore needs its old last
        block, with its new bytes.  Returns (Tag, State): the tag with the
        listed values replaced (patch_tag), and a state of n' blocks under the
        same f_key and alpha_key, encrypted and signed with a fresh IV as
        encode returns it.  Neither argument is modified."""
        self._check()
        st = self._open_state(state)
        n_new, indices, data = self._plan_update(st, blocks, length)
        raw = encode_blocks_many(self.prime, self.sectors, [(st.f_key, st.alpha_key, indices, data)])[0]
        return self._finish_update(tag, st, n_new, indices, raw)

    def update_file(self, tag, state, file, changed):
        """update() from the new file itself: `changed` is a list of (offset,
        nbytes) ranges of the NEW file that differ from the tagged one.  The
        new length is the file's; the blocks re-tagged are those the ranges
        touch plus the ones update()'s length rule demands.  The file is read
        from its start and its position is left where it was."""
        self._check()
        fb = FileBuffer(file, from_start=True)
        try:
            blocks, length = _blocks.file_blocks(self._block_bytes(), state.n, fb, changed)
        finally:
            fb.restore()
            fb.close()
        return self.update(tag, state, blocks, length)

    def update_many(self, items):
        """update(tag, state, blocks, length) of every item of `items` in one
        batched GPU call (hb_cxx_encode_blocks_many): [(Tag, State), ...],
        exactly what a loop of update() returns, and the HeartbeatError of the
        first item a loop would raise it for, before any GPU work.  Items whose
        key length differs from the first one's, and a batch of fewer than
        CXX_UPDATE_MANY_MIN items, go through update() one by one."""
        items = [(tag, state, list(blocks), length) for tag, state, blocks, length in items]
        self._check()
        pre = []
        for tag, state, blocks, length in items:
            st = self._open_state(state)
            pre.append((st,) + self._plan_update(st, blocks, length))
        if len(items) < CXX_UPDATE_MANY_MIN:
            return [self.update(*item) for item in items]
        klen = (len(_kb(pre[0][0].f_key)), len(_kb(pre[0][0].alpha_key))) if pre else None
        batch = [k for k, t in enumerate(pre) if (len(_kb(t[0].f_key)), len(_kb(t[0].alpha_key))) == klen
                 and klen[0] == klen[1]]
        raws = encode_blocks_many(self.prime, self.sectors,
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
        """l = (unsigned int)(check_fraction * n) indices, v limit p (:704-729)."""
        s = state._copy()   # `state s = s_enc` (:706)
        if s.encrypted and not s._check_sig_and_decrypt(self.k_enc, self.k_mac):
            raise HeartbeatError("Signature check or decryption failed in generating challenge.  "
                                 "State of remote file cannot be verified.")
        l = int(self.check_fraction * int(s.n)) & 0xffffffff
        return Challenge(l, self.prime, _random_bytes(KEY_SIZE))

    def prove(self, file, chal, tag):
        """mu_j, sigma over the challenged blocks (:731-789)."""
        self._check()
        p = self.prime
        S = self.sectors
        ntags = len(tag)
        if ntags == 0:
            raise HeartbeatError("tag is empty")
        proof = Proof()
        chunks = int(chal.chunks)
        if chunks <= 0:
            proof.mu = [0] * S
            proof.sigma = 0
            return proof
        tarr = np.frombuffer(tag.raw(p), dtype=np.uint8)
        key = _kb(chal.key)
        vmax = _native.be(int(chal.v_max))
        # absolute offsets from the start of the file, as the reference's
        # f.seek(pos) before every read (shacham_waters_private.cxx:763-764)
        fb = FileBuffer(file, from_start=True)
        try:
            proof.mu, proof.sigma = multi.prove_shards(p, S, key, chunks, vmax, tarr.ctypes.data, ntags,
                                                       fb.addr, fb.len, _native.HB_PRF_CXX, multi.devices())
        finally:
            fb.restore()
            fb.close()
        return proof

    def verify(self, proof, chal, state):
        """sigma == sum v_i f(idx_i) + sum alpha(j) mu_j mod p (:791-842);
        False when the state does not authenticate or mu has the wrong length,
        None for arguments of the wrong types (Swizzle.hxx:704-707)."""
        if not (isinstance(proof, Proof) and isinstance(chal, Challenge) and isinstance(state, State)):
            return None
        s = state._copy()   # `state s = s_enc` (:796)
        if s.encrypted and not s._check_sig_and_decrypt(self.k_enc, self.k_mac):
            return False
        self._check()
        p = self.prime
        S = self.sectors
        w = _native.width_of(p)
        mu = list(proof.mu)
        if len(mu) != S:
            return False
        chunks = max(int(chal.chunks), 0)
        if chunks and int(s.n) <= 0:
            raise HeartbeatError("state has no chunks")
        mub = b"".join((int(m) % p).to_bytes(w, "big") for m in mu)
        vmax = _native.be(int(chal.v_max)) if chunks else b"\x01"
        rhs = ctypes.create_string_buffer(w)
        ctx = multi.primary_context()
        pb = _native.be(p)
        fk, ak, ck = _kb(s.f_key), _kb(s.alpha_key), _kb(chal.key)
        with ctx.lock:
            ctx.check(_native.lib().hb_cxx_verify_rhs(ctx.h, pb, len(pb), S, fk, ak, len(fk),
                                                      int(s.n), ck, len(ck), chunks, vmax,
                                                      len(vmax), mub, rhs))
        return int(proof.sigma) == int.from_bytes(rhs.raw, "big")

    def prove_many(self, items):
        """prove() of every (file, chal, tag) of `items` in one batched GPU
        call (hb_cxx_prove_many): [Proof, ...], exactly what a loop of prove()
        (:731-789) returns, in order -- a zero proof for chunks <= 0 -- and
        HeartbeatError("tag is empty") at the first item a loop would raise it
        for.  Every item is checked before any GPU work, so a failing item
        costs no launch.  Files are read at absolute offsets and their
        position is restored.  Items whose key length differs from the
        batch's majority go through prove() one by one, and so do challenges
        that prove() would shard over several GPUs and a batch of fewer than
        CXX_PROVE_MANY_MIN items."""
        items = list(items)
        S = self.sectors
        out = [None] * len(items)
        cand = []
        for i, (file, chal, tag) in enumerate(items):
            self._check()
            if len(tag) == 0:
                raise HeartbeatError("tag is empty")
            if int(chal.chunks) <= 0:
                out[i] = Proof()
                out[i].mu = [0] * S
                out[i].sigma = 0
            else:
                cand.append(i)
        ndev = len(multi.devices())
        lens = [len(_kb(items[i][1].key)) for i in cand]
        major = max(set(lens), key=lens.count) if lens else 0
        batch = [i for i, kl in zip(cand, lens) if kl == major and
                 multi.shard_count(ndev, int(items[i][1].chunks), multi.MIN_SHARD_CHUNKS) == 1]
        if len(batch) < CXX_PROVE_MANY_MIN:
            batch = []
        if batch:
            res = prove_files(self.prime, S, [(items[i][1].key, int(items[i][1].chunks), int(items[i][1].v_max),
                                               items[i][2], items[i][0]) for i in batch])
            for i, (mu, sigma) in zip(batch, res):
                out[i] = Proof()
                out[i].mu, out[i].sigma = mu, sigma
        for i, (file, chal, tag) in enumerate(items):
            if out[i] is None:
                out[i] = self.prove(file, chal, tag)
        return out

    def verify_many(self, items):
        """verify() of every (proof, chal, state) of `items` in one batched
        GPU call (hb_cxx_verify_rhs_many): exactly what a loop of verify()
        (:791-842) returns, in order -- None for arguments of the wrong types,
        False for a state that does not authenticate or len(mu) != sectors --
        and HeartbeatError("state has no chunks") as the loop would raise it.
        Every item is checked before any GPU work, on a copy of its state.
        Items whose key lengths differ from the batch's majority go through
        verify() one by one, and so does a batch of fewer than
        CXX_VERIFY_MANY_MIN items."""
        items = list(items)
        S = self.sectors
        out = [None] * len(items)
        pre = {}
        for i, (proof, chal, state) in enumerate(items):
            if not (isinstance(proof, Proof) and isinstance(chal, Challenge) and isinstance(state, State)):
                continue   # None
            s = state._copy()   # `state s = s_enc` (:796)
            if s.encrypted and not s._check_sig_and_decrypt(self.k_enc, self.k_mac):
                out[i] = False
                continue
            self._check()
            mu = list(proof.mu)
            if len(mu) != S:
                out[i] = False
                continue
            chunks = max(int(chal.chunks), 0)
            if chunks and int(s.n) <= 0:
                raise HeartbeatError("state has no chunks")
            pre[i] = (_kb(s.f_key), _kb(s.alpha_key), int(s.n), _kb(chal.key), chunks,
                      int(chal.v_max) if chunks else 1, mu)
        lens = [(len(t[0]), len(t[1]), len(t[3])) for t in pre.values()]
        major = max(set(lens), key=lens.count) if lens else None
        batch = [i for i, kl in zip(pre, lens) if kl == major and kl[0] == kl[1]]
        if len(batch) < CXX_VERIFY_MANY_MIN:
            batch = []
        if batch:
            rhs = verify_rhs_many(self.prime, S, [pre[i] for i in batch])
            for i, r in zip(batch, rhs):
                out[i] = int(items[i][0].sigma) == r
        for i in pre:
            if out[i] is None:
                out[i] = self.verify(*items[i])
        return out

    @staticmethod
    def prove_mixed(items):
        """b.prove(file, chal, tag) of every (beat, file, chal, tag) of
        `items`, with any mix of beats -- primes, sector counts, challenge key
        lengths -- in one batched GPU call (hb_cxx_prove_mixed): the proofs a
        storage node owes to many owners, each of whom drew their own prime
        (init, shacham_waters_private.cxx:596-624).  [Proof, ...], exactly
        what [b.prove(f, c, t) for b, f, c, t in items] returns (:731-789 per
        item) -- a zero proof for chunks <= 0 -- and
        HeartbeatError("tag is empty") at the first item a loop would raise it
        for.  Every item is checked before any GPU work.  Files are read at
        absolute offsets and their position is restored.  Challenges that
        prove() would shard over several GPUs go through prove(), and so does
        a batch of fewer than CXX_PROVE_MANY_MIN items."""
        items = list(items)
        out = [None] * len(items)
        cand = []
        for i, (beat, file, chal, tag) in enumerate(items):
            beat._check()
            if len(tag) == 0:
                raise HeartbeatError("tag is empty")
            if int(chal.chunks) <= 0:
                out[i] = Proof()
                out[i].mu = [0] * int(beat.sectors)
                out[i].sigma = 0
            else:
                cand.append(i)
        ndev = len(multi.devices())
        batch = [i for i in cand
                 if multi.shard_count(ndev, int(items[i][2].chunks), multi.MIN_SHARD_CHUNKS) == 1]
        if len(batch) < CXX_PROVE_MANY_MIN:
            batch = []
        if batch:
            res = prove_files_mixed(
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
        (hb_cxx_verify_rhs_mixed): an auditor checking the proofs of several
        owners.  Each state is authenticated and decrypted with its own beat's
        keys, on a copy.  Exactly what a loop of verify() (:791-842) returns,
        in order -- None for arguments of the wrong types, False for a state
        that does not authenticate under its own beat or len(mu) != sectors
        -- and HeartbeatError("state has no chunks") as the loop would raise
        it.  Every item is checked before any GPU work.  A batch of fewer than
        CXX_VERIFY_MANY_MIN items goes through verify()."""
        items = list(items)
        out = [None] * len(items)
        pre = {}
        for i, (beat, proof, chal, state) in enumerate(items):
            if not (isinstance(proof, Proof) and isinstance(chal, Challenge) and isinstance(state, State)):
                continue   # None
            s = state._copy()   # `state s = s_enc` (:796)
            if s.encrypted and not s._check_sig_and_decrypt(beat.k_enc, beat.k_mac):
                out[i] = False
                continue
            beat._check()
            S = int(beat.sectors)
            mu = list(proof.mu)
            if len(mu) != S:
                out[i] = False
                continue
            chunks = max(int(chal.chunks), 0)
            if chunks and int(s.n) <= 0:
                raise HeartbeatError("state has no chunks")
            pre[i] = (int(beat.prime), S, _kb(s.f_key), _kb(s.alpha_key), int(s.n), _kb(chal.key), chunks,
                      int(chal.v_max) if chunks else 1, mu)
        batch = [i for i, t in pre.items() if len(t[2]) == len(t[3])]
        if len(batch) < CXX_VERIFY_MANY_MIN:
            batch = []
        if batch:
            rhs = verify_rhs_mixed([pre[i] for i in batch])
            for i, r in zip(batch, rhs):
                out[i] = int(items[i][1].sigma) == r
        for i in pre:
            if out[i] is None:
                beat, proof, chal, state = items[i]
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


# Fewest files Swizzle.encode_many sends through hb_cxx_encode_many; below it
# the files go through encode() one by one.  Already one file is ahead in the
# batch's three launches (1024-bit, S = 10, 1 MiB: B's slowest round beats A's
# fastest device-resident and from host memory, and by 2x and 3x at two and
# three files: the 1-, 2- and 3-file rows of scripts/cxx_many_rate.py,
# profiles/many/cxx_many_rate.json) -- the single cxx encode
# is an alpha launch, a Montgomery pass and the engine launch with a
# synchronise of its own -- so every non-empty list takes the batch.
CXX_ENCODE_MANY_MIN = 1


def encode_files(p, sectors, keys, files):
    """Batched GPU encode (hb_cxx_encode_many) of many file objects / buffers
    with the cxx prf, file i under keys[i] = (f_key, alpha_key): [(Tag, number
    of blocks), ...].  Each file is read from its current position to EOF and
    left there, as by Swizzle.encode; all keys of a batch have one length.
    Every file is opened before any GPU work; if one cannot be read, the files
    before it are left at EOF as the loop leaves them and its error is raised.
    Runs on multi.primary_context() (a batch is not spread over several
    GPUs)."""
    return _many.encode_files("hb_cxx_encode_many", Tag, p, sectors, keys, files, open_first=True)


# Fewest files Swizzle.encode_mixed sends through hb_cxx_encode_mixed; below it
# the items go through encode() one by one: the smallest file count at which
# the mixed call's slowest round beats the loop's fastest.  Already one file is
# ahead (1024-bit, S = 10, 1 MiB: 0.22-0.28 against 0.32-0.35 ms
# device-resident, 0.29-0.36 against 0.48-0.51 from host memory; 2.7x and 2.5x
# at two files, 3.7x and 3.2x at three: the --files 1, 2 and 3 rows of
# scripts/encode_mixed_rate.py --cxx, profiles/many/cxx_encode_mixed_rate.json,
# DESIGN.md 5.3i), as with CXX_ENCODE_MANY_MIN, so every non-empty list takes
# the mixed call.
CXX_ENCODE_MIXED_MIN = 1


def encode_files_mixed(items):
    """Batched GPU encode (hb_cxx_encode_mixed) of the files of many owners
    with the cxx prf: `items` is a list of (p, sectors, f_key, alpha_key,
    file), every file under its own prime, sector count and key length; returns
    [(Tag, number of blocks), ...], what hb_encode(HB_PRF_CXX) gives per item
    (shacham_waters_private.cxx:638-702).  File handling as encode_files:
    every file is opened before any GPU work; if one cannot be read, the files
    before it are left at EOF as the loop leaves them and its error is raised.
    Runs on multi.primary_context()."""
    return _many.encode_files_mixed(items, "hb_cxx_encode_mixed", Tag, open_first=True)


# Fewest items Swizzle.update_many sends through one hb_cxx_encode_blocks_many;
# below it the items go through update() one by one.  One item is the same
# call either way (update() itself is hb_cxx_encode_blocks_many with one
# descriptor), so the batch starts at two: 1024-bit, S = 10, 4 blocks per file,
# two files in one call take 0.195-0.214 ms from host memory where one file
# takes 0.165-0.177 (0.199-0.222 against 0.173-0.187 device-resident), the
# files rows of scripts/cxx_blocks_rate.py, profiles/many/cxx_blocks_rate.json,
# DESIGN.md 5.3l.
CXX_UPDATE_MANY_MIN = 2


def encode_blocks_many(p, sectors, items):
    """Batched GPU tags of listed blocks with the cxx prf
    (hb_cxx_encode_blocks_many): `items` is a list of (f_key, alpha_key,
    indices, data) with each file's listed blocks back to back in `data` and
    every index below 2^32; returns one uint8 array of tag images per item.
    Runs on multi.primary_context()."""
    return _many.encode_blocks_many(p, sectors, items, native="hb_cxx_encode_blocks_many")


# Fewest proofs Swizzle.prove_many sends through hb_cxx_prove_many, and
# Swizzle.verify_many through hb_cxx_verify_rhs_many; below them the items go
# through prove() / verify() one by one.  Already one proof is ahead in the
# batch (1024-bit, S = 10, a 1 MiB file, B's slowest round against A's fastest:
# prove 1.37x device-resident and 1.26x from host memory at check_fraction 1.0,
# 1.84x and 1.44x at 0.3; verify 1.43x and 1.62x; from 2.3x at two proofs and
# 3.1x at three: the 1-, 2- and 3-proof rows of scripts/cxx_pv_many_rate.py,
# profiles/many/cxx_pv_many_rate.json) -- the single cxx calls
# take none of the fused paths: a prove is a PRF launch, a weighted sum and
# their synchronisation, a verify up to four PRF launches, a Montgomery pass
# and a sum -- so every non-empty list takes the batch.  The static
# prove_mixed / verify_mixed (hb_cxx_prove_mixed, hb_cxx_verify_rhs_mixed) use
# the same two constants: one proof through the mixed call is ahead of one
# single call in all six shapes as well (B's slowest round against A's fastest
# 1.11x to 1.47x, from 1.9x at two proofs and 2.7x at three: the --proofs 1, 2
# and 3 rows of scripts/cxx_mixed_many_rate.py,
# profiles/many/cxx_mixed_many_rate.json).
CXX_PROVE_MANY_MIN = 1
CXX_VERIFY_MANY_MIN = 1


def prove_files(p, sectors, items):
    """Batched GPU prove (hb_cxx_prove_many) of many challenges with the cxx
    prf: `items` is a list of (chal_key, chunks, v_max, tag, file) with a Tag
    and a file object / buffer each; returns [(mu list, sigma), ...], what
    hb_prove(HB_PRF_CXX) gives per item (shacham_waters_private.cxx:731-789).
    Every file is read whole, from its start, and its position is left where
    it was, as by Swizzle.prove.  Every item is checked before any GPU work.
    All challenge keys of a batch have one length.  Runs on
    multi.primary_context() (a batch is not spread over several GPUs)."""
    return _many.prove_files("hb_cxx_prove_many", p, sectors, items)


def verify_rhs_many(p, sectors, items):
    """Batched right-hand sides (hb_cxx_verify_rhs_many) of many proofs with
    the cxx prf: `items` is a list of (f_key, alpha_key, state_chunks,
    chal_key, chunks, v_max, mu_list) with decrypted state keys; returns the
    list of ints that hb_cxx_verify_rhs gives per item
    (shacham_waters_private.cxx:791-842).  Every item is checked before any
    GPU work.  All f_keys and alpha_keys of a batch have one length, all
    challenge keys one length.  Runs on multi.primary_context() (a batch is
    not spread over several GPUs)."""
    # exactly `sectors` mu values, as the message says
    return _many.verify_rhs_many("hb_cxx_verify_rhs_many", p, sectors, items, exact_mu=True)


def prove_files_mixed(items):
    """Batched GPU prove (hb_cxx_prove_mixed) of the challenges of many owners
    with the cxx prf: `items` is a list of (p, sectors, chal_key, chunks,
    v_max, tag, file), each under its own prime, sector count and key length;
    returns [(mu list, sigma), ...], what hb_prove(HB_PRF_CXX) gives per item
    (shacham_waters_private.cxx:731-789).  File handling and checks as
    prove_files.  Runs on multi.primary_context()."""
    return _many.prove_files_mixed(items, native="hb_cxx_prove_mixed")


def verify_rhs_mixed(items):
    """Batched right-hand sides (hb_cxx_verify_rhs_mixed) of the proofs of
    many owners with the cxx prf: `items` is a list of (p, sectors, f_key,
    alpha_key, state_chunks, chal_key, chunks, v_max, mu_list) with decrypted
    state keys, each under its own prime, sector count and key lengths;
    returns the list of ints that hb_cxx_verify_rhs gives per item
    (shacham_waters_private.cxx:791-842).  A proof has exactly `sectors` mu
    values.  Runs on multi.primary_context()."""
    return _many.verify_rhs_mixed(items, native="hb_cxx_verify_rhs_mixed", exact_mu=True)


# The extension module's path (cxx/Swizzle.hxx:738, imported as
# heartbeat.Swizzle): pickles name heartbeat.Swizzle.<type>, which the repo's
# heartbeat/ package re-exports.
for _c in (Swizzle, Tag, State, Challenge, Proof):
    _c.__module__ = "heartbeat.Swizzle"
del _c
