"""MerkleHelper (heartbeat/Merkle/Merkle.py:447-515) over the GPU KeyedPRF.

The Merkle scheme picks, for every challenge seed, the chunk of the file that
the challenge checks: ``KeyedPRF(seed, filesz - chunksz + 1).eval(0)``
(Merkle.py:502-503), and its leaf is HMAC-SHA256(seed, chunk)
(:505-515).  ``Merkle.encode`` does this for 256 seeds of an HMAC chain
(:357-361).  Here the positions of any number of seeds come from ONE kernel
launch (``hb_merkle_offsets``: a lane per seed, each expanding its own AES
key schedule), and for device-resident files the leaves too
(``hb_merkle_chunk_hmacs``: a lane per chunk).  Host files are hashed on the
host, reading the chunk through the file object as the reference does: the
bytes are already there, and one SHA-256 stream is serial.

The scheme itself (heartbeat/Merkle/Merkle.py:45-444): ``Challenge``, ``Tag``,
``State``, ``Proof`` and ``Merkle``.  ``Merkle.encode`` runs the seed chain,
the n leaves and the tree on the GPU (hb_merkle_encode_many: three launches,
no host round trip between them), ``Merkle.prove`` the challenged leaf
(hb_merkle_leaves_many); ``encode_many`` / ``encode_mixed`` / ``prove_many``
put any number of files or proofs, of one owner or of many, into the same
launches.  ``gen_challenge``, ``verify`` and the state's HMAC are host code: a
verify is order + 1 small hashes.

Differences from the reference, all on inputs it fails on:
  * ``encode`` with n < 1 raises HeartbeatError (the reference fails inside
    math.log), and with n > 65536 too (the GPU path's cap);
  * a ``filesz`` beyond the file raises HeartbeatError ("chunk past the end of
    the data"; the reference's read loop never ends);
  * a challenge seed that is no AES key (16, 24 or 32 bytes) raises
    HeartbeatError (the reference raises ValueError from its cipher).
"""
import ctypes
import hashlib
import hmac
import os
import time

import numpy as np

from .. import _native, multi
from .._filebuf import FileBuffer
from ..exc import HeartbeatError
from ..util import hb_encode, hb_decode
from .MerkleTree import MerkleTree, MerkleBranch, MerkleLeaf

DEFAULT_CHUNK_SIZE = 8192     # Merkle.py:38
DEFAULT_BUFFER_SIZE = 65536   # Merkle.py:39
DEFAULT_CHALLENGE_COUNT = 256   # Merkle.py:40
DEFAULT_KEY_SIZE = 32         # Merkle.py:41


def _seed_block(seeds):
    seeds = [bytes(s) for s in seeds]
    n = len(seeds)
    if n == 0:
        return b"", 0, 0
    sl = len(seeds[0])
    if any(len(s) != sl for s in seeds):
        raise HeartbeatError("seeds of one batch must have one length")
    return b"".join(seeds), sl, n


class MerkleHelper(object):
    """Helper functions of the Merkle scheme (Merkle.py:447-515)."""

    @staticmethod
    def get_next_seed(key, seed):
        """HMAC-SHA256(key, seed): the next seed of the chain (Merkle.py:451-460)."""
        return hmac.new(key, seed, hashlib.sha256).digest()

    @staticmethod
    def seed_chain(key, seed, n):
        """The n leaf seeds Merkle.encode derives from the state seed
        (Merkle.py:357-361): s_1 = next(key, seed), s_{k+1} = next(key, s_k)."""
        out = []
        s = seed
        for _ in range(n):
            s = MerkleHelper.get_next_seed(key, s)
            out.append(s)
        return out

    @staticmethod
    def get_file_hash(file, seed, bufsz=DEFAULT_BUFFER_SIZE):
        """HMAC-SHA256(seed, rest of the file) (Merkle.py:462-478): a host read loop."""
        h = hmac.new(seed, None, hashlib.sha256)
        while True:
            buffer = file.read(bufsz)
            h.update(buffer)
            if len(buffer) != bufsz:
                break
        return h.digest()

    @staticmethod
    def chunk_offsets(seeds, filesz, chunksz=DEFAULT_CHUNK_SIZE):
        """Chunk positions KeyedPRF(seed, filesz - chunk + 1).eval(0) of many
        seeds, chunk = min(chunksz, filesz) (Merkle.py:500-503), in one GPU
        launch.  Seeds are AES keys: 16, 24 or 32 bytes."""
        blob, sl, n = _seed_block(seeds)
        if n == 0:
            return []
        out = np.zeros(n, dtype=np.uint64)
        ctx = multi.primary_context()
        with ctx.lock:
            ctx.check(_native.lib().hb_merkle_offsets(ctx.h, blob, sl, n, int(filesz), int(chunksz),
                                                      out.ctypes.data))
        return [int(x) for x in out]

    @staticmethod
    def get_chunk_hash(file, seed, filesz=None, chunksz=DEFAULT_CHUNK_SIZE, bufsz=DEFAULT_BUFFER_SIZE):
        """The leaf of one seed (Merkle.py:480-515): HMAC-SHA256(seed, the
        chunksz bytes at KeyedPRF(seed, filesz - chunksz + 1).eval(0)).
        Leaves the file after the chunk, as the reference's reads do."""
        return MerkleHelper.get_chunk_hashes(file, [seed], filesz, chunksz, bufsz)[0]

    @staticmethod
    def get_chunk_hashes(file, seeds, filesz=None, chunksz=DEFAULT_CHUNK_SIZE, bufsz=DEFAULT_BUFFER_SIZE):
        """get_chunk_hash for many seeds: positions in one GPU launch, leaves
        hashed on the host from the file object (seek + reads of bufsz)."""
        if filesz is None:
            file.seek(0, 2)
            filesz = file.tell()
        if filesz < chunksz:
            chunksz = filesz
        offs = MerkleHelper.chunk_offsets(seeds, filesz, chunksz)
        out = []
        for seed, i in zip(seeds, offs):
            file.seek(i)
            h = hmac.new(seed, None, hashlib.sha256)
            left, bs = chunksz, bufsz
            while True:
                if left < bs:
                    bs = left
                buffer = file.read(bs)
                h.update(buffer)
                left -= len(buffer)
                if left == 0:
                    break
                if not buffer:
                    # the reference loops forever here (a filesz larger than the file)
                    raise HeartbeatError("file shorter than filesz")
            out.append(h.digest())
        return out

    @staticmethod
    def device_chunk_hashes(data_ptr, length, seeds, filesz=None, chunksz=DEFAULT_CHUNK_SIZE):
        """Leaves of many seeds over a DEVICE-resident file (hb_device_malloc'd
        pointer, `length` bytes): positions and HMACs both on the GPU.
        Returns (offsets, digests)."""
        filesz = length if filesz is None else int(filesz)
        if filesz < chunksz:
            chunksz = filesz
        offs = MerkleHelper.chunk_offsets(seeds, filesz, chunksz)
        blob, sl, n = _seed_block(seeds)
        if n == 0:
            return [], []
        oarr = np.asarray(offs, dtype=np.uint64)
        dig = ctypes.create_string_buffer(32 * n)
        ctx = multi.primary_context()
        with ctx.lock:
            ctx.check(_native.lib().hb_merkle_chunk_hmacs(ctx.h, blob, sl, n, data_ptr, int(length),
                                                          oarr.ctypes.data, int(chunksz), dig))
        raw = dig.raw
        return offs, [raw[32 * k:32 * (k + 1)] for k in range(n)]


MerkleHelper.__module__ = "heartbeat.Merkle.Merkle"   # the reference's path (repo heartbeat/ package)


class Challenge(object):
    """A challenge: the seed that places and keys the chunk's HMAC, and the
    index of the tree's branch (Merkle.py:45-83)."""

    def __init__(self, seed=0, index=0):
        self.seed = seed
        self.index = index

    def __eq__(self, other):
        return isinstance(other, Challenge) and self.seed == other.seed and self.index == other.index

    def todict(self):
        return {'seed': hb_encode(self.seed), 'index': self.index}

    @staticmethod
    def fromdict(dict):
        return Challenge(hb_decode(dict['seed']), dict['index'])


class Tag(object):
    """The file tag: the tree without its leaf payloads, the chunk size and
    the file size the positions were drawn for (Merkle.py:87-131)."""

    def __init__(self, tree=MerkleTree(), chunksz=DEFAULT_CHUNK_SIZE, filesz=None):
        self.tree = tree
        self.chunksz = chunksz
        self.filesz = filesz

    def __eq__(self, other):
        return (isinstance(other, Tag) and self.tree == other.tree and
                self.chunksz == other.chunksz and self.filesz == other.filesz)

    def todict(self):
        return {'tree': self.tree.todict(), 'chunksz': self.chunksz, 'filesz': self.filesz}

    @staticmethod
    def fromdict(dict):
        return Tag(MerkleTree.fromdict(dict['tree']), dict['chunksz'], dict['filesz'])


class State(object):
    """The mutable state of a file (Merkle.py:134-241): the seed and index of
    the last challenge issued, the number of challenges n, the tree's root, a
    timestamp and the HMAC that signs them.  As in the reference, the default
    timestamp is the time this module was imported, not the time of the call
    (a default argument is evaluated once): pass one to get another."""

    def __init__(self, index=0, seed=0, n=0, root=None, hmac=None, timestamp=time.time()):
        self.index = index
        self.seed = seed
        self.n = n
        self.root = root
        self.hmac = hmac
        self.timestamp = timestamp

    def __eq__(self, other):
        return (isinstance(other, State) and self.index == other.index and self.seed == other.seed and
                self.n == other.n and self.root == other.root and self.hmac == other.hmac and
                self.timestamp == other.timestamp)

    def todict(self):
        return {'index': self.index, 'seed': hb_encode(self.seed), 'n': self.n,
                'root': hb_encode(self.root), 'hmac': hb_encode(self.hmac),
                'timestamp': self.timestamp}

    @staticmethod
    def fromdict(dict):
        return State(dict['index'], hb_decode(dict['seed']), dict['n'], hb_decode(dict['root']),
                     hb_decode(dict['hmac']), dict['timestamp'])

    def get_hmac(self, key):
        """HMAC-SHA256 under `key` of str(index), seed, str(n), root and
        str(timestamp), in that order (Merkle.py:209-220)."""
        msg = (str(self.index).encode() + self.seed + str(self.n).encode() + self.root +
               str(self.timestamp).encode())
        return hmac.new(key, msg, hashlib.sha256).digest()

    def sign(self, key):
        self.hmac = self.get_hmac(key)

    def checksig(self, key):
        if self.get_hmac(key) != self.hmac:
            raise HeartbeatError("Signature invalid on state.")


class Proof(object):
    """A proof: the challenged leaf and its branch (Merkle.py:244-270)."""

    def __init__(self, leaf=MerkleLeaf(0, bytes()), branch=MerkleBranch(0)):
        self.leaf = leaf
        self.branch = branch

    def __eq__(self, other):
        return self.leaf == other.leaf and self.branch == other.branch

    def todict(self):
        return {'leaf': self.leaf.todict(), 'branch': self.branch.todict()}

    @staticmethod
    def fromdict(dict):
        return Proof(MerkleLeaf.fromdict(dict['leaf']), MerkleBranch.fromdict(dict['branch']))


class DeviceFile(object):
    """A file whose bytes are in GPU memory: `length` bytes at the device
    pointer `ptr` (hb_device_malloc).  Takes the place of the file object in
    encode / prove and their batches; seek and tell keep a position so that a
    call leaves it where it would leave a host file."""

    def __init__(self, ptr, length):
        self.ptr = int(ptr)
        self.len = int(length)
        self.pos = 0

    def seek(self, pos, whence=0):
        self.pos = int(pos) + (0, self.pos, self.len)[whence]
        return self.pos

    def tell(self):
        return self.pos


class _Source(object):
    """The bytes of one file of a batch: a DeviceFile's pointer, or a host
    file's whole contents from offset 0 (the chunk positions are absolute)."""

    def __init__(self, file):
        self.file = file
        self.fb = None
        self.on_device = isinstance(file, DeviceFile)
        if self.on_device:
            self.addr, self.len = (file.ptr if file.len else None), file.len
        else:
            self.fb = FileBuffer(file, from_start=True)
            self.addr, self.len = self.fb.addr, self.fb.len

    def leave_at(self, pos):
        try:
            self.file.seek(int(pos))
        except Exception:
            pass

    def close(self):
        if self.fb is not None:
            self.fb.close()


def _open_all(files):
    srcs = []
    try:
        for f in files:
            srcs.append(_Source(f))
    except BaseException:
        for s in srcs:
            s.close()
        raise
    if len({s.on_device for s in srcs}) > 1:
        for s in srcs:
            s.close()
        raise HeartbeatError("device-resident and host files cannot share a batch")
    return srcs


_CHAIN_FLAGS = {None: 0, "host": _native.HB_MERKLE_CHAIN_HOST, "device": _native.HB_MERKLE_CHAIN_DEVICE}


def encode_batch(items, chain=None, leaves=False):
    """Merkle.encode of every item = (merkle, file, n, seed, chunksz, filesz)
    in one hb_merkle_encode_many call; seed, chunksz and filesz may be None as
    in Merkle.encode.  Returns [(tag, state), ...], or with leaves=True
    [(tag, state, leaf blobs, chunk positions), ...].  chain: "host" or
    "device" forces where the seed chains run (None: the runtime decides by
    the number of files).  Every file is left at its last leaf's position plus
    the chunk, where the reference's last read ends."""
    items = list(items)
    plan = []
    for merkle, file, n, seed, chunksz, filesz in items:
        n = int(n)
        if n < 1 or n > _native.HB_MERKLE_MAX_N:
            raise HeartbeatError("n must be in 1..65536 on the GPU path")
        plan.append((merkle, n, os.urandom(DEFAULT_KEY_SIZE) if seed is None else bytes(seed), chunksz, filesz))
    if not plan:
        return []
    srcs = _open_all([it[1] for it in items])
    try:
        descs = (_native.MerkleEncodeDesc * len(plan))()
        keep = []
        for d, src, (merkle, n, seed, chunksz, filesz) in zip(descs, srcs, plan):
            filesz = src.len if filesz is None else int(filesz)
            if chunksz is None:
                if merkle.check_fraction is not None:
                    chunksz = int(merkle.check_fraction * filesz)
                else:
                    chunksz = DEFAULT_CHUNK_SIZE
            if filesz < 0 or chunksz < 0:
                raise HeartbeatError("filesz and chunksz must not be negative")
            if filesz > src.len:
                raise HeartbeatError("chunk past the end of the data")
            key = bytes(merkle.key)
            order = (n - 1).bit_length()
            nodes = np.zeros((2 << order) * 32, dtype=np.uint8)
            blobs = np.zeros(n * 32, dtype=np.uint8)
            offs = np.zeros(n, dtype=np.uint64)
            d.key, d.key_len, d.seed, d.seed_len = key, len(key), seed, len(seed)
            d.n, d.filesz, d.chunksz = n, filesz, int(chunksz)
            d.data, d.len = src.addr, src.len
            d.nodes_out, d.offsets_out = nodes.ctypes.data, offs.ctypes.data
            d.leaves_out = blobs.ctypes.data if leaves else None
            keep.append((key, seed, n, order, chunksz, filesz, nodes, blobs, offs))
        flags = _CHAIN_FLAGS[chain] | (_native.HB_DATA_ON_DEVICE if srcs[0].on_device else 0)
        ctx = multi.primary_context()
        with ctx.lock:
            ctx.check(_native.lib().hb_merkle_encode_many(ctx.h, descs, len(plan), flags))
        out = []
        for src, (key, seed, n, order, chunksz, filesz, nodes, blobs, offs) in zip(srcs, keep):
            tree = MerkleTree._from_raw(nodes.tobytes(), order, n)
            state = State(0, seed, n)
            state.root = tree.get_root()
            state.sign(key)
            tag = Tag(tree, chunksz, filesz)
            src.leave_at(int(offs[-1]) + min(int(chunksz), filesz))
            if leaves:
                raw = blobs.tobytes()
                out.append((tag, state, [raw[32 * k:32 * k + 32] for k in range(n)], [int(x) for x in offs]))
            else:
                out.append((tag, state))
        return out
    finally:
        for s in srcs:
            s.close()


def prove_batch(items):
    """Merkle.prove of every item = (file, challenge, tag) in one
    hb_merkle_leaves_many call: [Proof, ...].  Every file is left after its
    chunk."""
    items = list(items)
    if not items:
        return []
    for _, chal, _ in items:
        if len(bytes(chal.seed)) not in (16, 24, 32):
            raise HeartbeatError("AES key must be either 16, 24, or 32 bytes long")
    srcs = _open_all([it[0] for it in items])
    try:
        n = len(items)
        descs = (_native.MerkleLeafDesc * n)()
        blobs = np.zeros(n * 32, dtype=np.uint8)
        offs = np.zeros(n, dtype=np.uint64)
        keep = []
        for i, (d, src, (_, chal, tag)) in enumerate(zip(descs, srcs, items)):
            seed = bytes(chal.seed)
            filesz = src.len if tag.filesz is None else int(tag.filesz)
            chunksz = int(tag.chunksz)
            if filesz < 0 or chunksz < 0:
                raise HeartbeatError("filesz and chunksz must not be negative")
            if filesz > src.len:
                raise HeartbeatError("chunk past the end of the data")
            d.seed, d.seed_len, d.filesz, d.chunksz = seed, len(seed), filesz, chunksz
            d.data, d.len = src.addr, src.len
            d.leaf_out = blobs.ctypes.data + 32 * i
            d.offset_out = offs.ctypes.data + 8 * i
            keep.append((seed, min(chunksz, filesz)))
        ctx = multi.primary_context()
        with ctx.lock:
            ctx.check(_native.lib().hb_merkle_leaves_many(
                ctx.h, descs, n, _native.HB_DATA_ON_DEVICE if srcs[0].on_device else 0))
        raw = blobs.tobytes()
        out = []
        for i, (src, (_, chal, tag)) in enumerate(zip(srcs, items)):
            src.leave_at(int(offs[i]) + keep[i][1])
            out.append(Proof(MerkleLeaf(chal.index, raw[32 * i:32 * i + 32]), tag.tree.get_branch(chal.index)))
        return out
    finally:
        for s in srcs:
            s.close()


class Merkle(object):
    """The Merkle heartbeat (Merkle.py:273-444).  The owner holds a key;
    ``encode`` derives n leaf seeds from it by an HMAC chain, hashes a
    pseudo-randomly placed chunk of the file under each and keeps the root of
    the tree over them in a signed state; every challenge reveals the next
    seed of the chain, and the server answers with that chunk's HMAC and the
    leaf's branch."""

    def __init__(self, check_fraction=None, key=None):
        self.key = os.urandom(DEFAULT_KEY_SIZE) if key is None else key
        self.check_fraction = check_fraction

    def __eq__(self, other):
        return isinstance(other, Merkle) and self.key == other.key

    def todict(self):
        return {'key': hb_encode(self.key), 'check_fraction': self.check_fraction}

    @staticmethod
    def fromdict(dict):
        return Merkle(dict['check_fraction'], hb_decode(dict['key']))

    def get_public(self):
        """A Merkle without the key (b''): what the server holds."""
        return Merkle(self.check_fraction, b'')

    def encode(self, file, n=DEFAULT_CHALLENGE_COUNT, seed=None, chunksz=None, filesz=None):
        """(tag, state) of `file` for n challenges (Merkle.py:323-367): the
        seed chain, the n leaves and the tree in three GPU launches.  seed:
        the root seed (default: 32 random bytes); chunksz: bytes checked per
        challenge (default: check_fraction of the file, else 8192; a chunk
        larger than the file is the whole file); filesz: default, the file's
        length.  `file`: an object with read/seek/tell, or a DeviceFile."""
        return encode_batch([(self, file, n, seed, chunksz, filesz)])[0]

    def encode_many(self, files, n=DEFAULT_CHALLENGE_COUNT, seeds=None, chunksz=None):
        """encode of every file in `files` under this key in one call:
        [(tag, state), ...], identical to a loop of encode.  seeds: one per
        file (default: random ones)."""
        files = list(files)
        seeds = [None] * len(files) if seeds is None else list(seeds)
        if len(seeds) != len(files):
            raise HeartbeatError("%d seeds for %d files" % (len(seeds), len(files)))
        return encode_batch([(self, f, n, s, chunksz, None) for f, s in zip(files, seeds)])

    @staticmethod
    def encode_mixed(items):
        """encode of the files of many owners in one call: items =
        (merkle, file, n, seed, chunksz), each file under its own Merkle, n
        and chunk size; [(tag, state), ...]."""
        return encode_batch([(m, f, n, s, c, None) for m, f, n, s, c in items])

    def gen_challenge(self, state):
        """The next challenge of `state`, which moves on by one seed and index
        and is signed again (Merkle.py:369-386).  Host code."""
        state.checksig(self.key)
        if state.index >= state.n:
            raise HeartbeatError("Out of challenges.")
        state.seed = MerkleHelper.get_next_seed(self.key, state.seed)
        chal = Challenge(state.seed, state.index)
        state.index += 1
        state.sign(self.key)
        return chal

    def prove(self, file, challenge, tag):
        """The proof for `challenge`: the HMAC of the challenged chunk (one
        GPU lane) and the leaf's branch out of the tag (Merkle.py:388-404)."""
        return prove_batch([(file, challenge, tag)])[0]

    @staticmethod
    def prove_many(items):
        """prove of every item = (file, challenge, tag) in one call, whatever
        files and owners they belong to: [Proof, ...]."""
        return prove_batch(items)

    def verify(self, proof, challenge, state):
        """True if `proof` answers `challenge` under the root in `state`
        (Merkle.py:406-420).  Host code: order + 1 small hashes."""
        state.checksig(self.key)
        if proof.leaf.index != challenge.index:
            return False
        return MerkleTree.verify_branch(proof.leaf, proof.branch, state.root)

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
