"""The OneHash heartbeat (heartbeat/OneHash/OneHash.py) with its responses and
seed chains on the GPU.

A challenge is a position in the file and a seed; its response is the SHA-256
of a chunk of the file at that position -- a tenth of the file, at most 1 KiB,
wrapped round at the end of the file -- followed by the seed
(OneHash.py:112-138).  ``generate_challenges`` derives ``num`` seeds from a
root seed by a hash chain under the owner's secret (:141-168), draws ``num``
positions from Python's module-level ``random`` (:170-189) and records every
response.  Every response is independent of the others, so a batch of them is
one kernel launch with a lane per response (``hb_onehash_meet_many``,
``hb_onehash_generate_many``; the chains of many files are a second launch
with a lane per file).

``pick_blocks`` and ``random_challenge`` stay on the module-level ``random``
with the reference's own call sequence: the generator's state after a call is
what it is there.

Two paths compute a response.  The GPU path takes challenges whose block is an
int inside the file and whose seed is ``bytes`` / ``bytearray`` of at most 64
bytes, in calls of at least ``hb_onehash_device_min_jobs()`` jobs.  Everything
else -- the blocks a foreign challenger may send (``file_size``,
``file_size + 1``, beyond, negative), longer seeds, seeds of other types, a
secret that is not bytes, small calls -- goes through the host path, which
performs the reference's own seeks and reads on the file object, so results
and exceptions are the reference's.  ``HB_ONEHASH_HOST=1`` sends everything to
the host path, ``HB_ONEHASH_DEVICE=1`` everything the GPU path can take to the
GPU whatever the job count.  There is no fall-back from the
GPU path: without the library or a GPU it raises HeartbeatError.

Beyond the reference's calls: ``meet_challenges`` (one file, many challenges),
``meet_many`` (many files), ``generate_challenges_many`` (many files) and
``from_device`` (a file already in GPU memory).
"""
import copy
import ctypes
import hashlib
import io
import os
import os.path
import random
import sys

import numpy as np

from .. import _native, multi
from .._filebuf import FileBuffer
from ..exc import HeartbeatError

MAX_CHUNK = 1024   # OneHash.py:120
MAX_GPU_SEED = _native.HB_ONEHASH_MAX_SEED_LEN


class Challenge(object):
    """A position in the file, a seed and -- on the challenger's side -- the
    expected response (OneHash.py:37-59)."""

    def __init__(self, block, seed):
        self.block = block
        self.seed = seed
        self.response = None

    @property
    def without_answer(self):
        """A copy with no ``response`` attribute: what goes to the other node."""
        sendable = copy.copy(self)
        del sendable.response
        return sendable


def _forced():
    """"host", "device" or None, by HB_ONEHASH_HOST / HB_ONEHASH_DEVICE."""
    if os.environ.get("HB_ONEHASH_HOST", "") not in ("", "0"):
        return "host"
    if os.environ.get("HB_ONEHASH_DEVICE", "") not in ("", "0"):
        return "device"
    return None


def _on_gpu(jobs):
    """Does a call of `jobs` GPU-eligible jobs go to the GPU?"""
    forced = _forced()
    if forced is not None:
        return forced == "device" and jobs > 0
    return jobs > 0 and jobs >= _native.lib().hb_onehash_device_min_jobs()


class _Sources(object):
    """The bytes of the files of one GPU call: device pointers, or host
    mappings of the file objects (closed on exit)."""

    def __init__(self, beats):
        self.beats = beats
        self.bufs = []
        if len({b._dev is not None for b in beats}) > 1:
            raise HeartbeatError("device-resident and host files cannot share a batch")
        self.on_device = bool(beats) and beats[0]._dev is not None

    def __enter__(self):
        out = []
        for b in self.beats:
            if self.on_device:
                out.append((b._dev if b.file_size else None, b.file_size))
            else:
                fb = FileBuffer(b.file_object, from_start=True)
                self.bufs.append(fb)
                if fb.len != b.file_size:
                    raise HeartbeatError("%d bytes in the file, %d when it was opened" % (fb.len, b.file_size))
                out.append((fb.addr, fb.len))
        return out

    def __exit__(self, *exc):
        for fb in self.bufs:
            fb.close()

    @property
    def flags(self):
        return _native.HB_DATA_ON_DEVICE if self.on_device else 0


class OneHash(object):
    """Hash challenges by which node A checks that node B holds a file
    (OneHash.py:62-233)."""

    def __init__(self, filepath, secret=None):
        """filepath: an existing file, opened for reading and kept open.
        secret: the owner's bytes under the seed chain; a node that only
        answers challenges needs none.  HeartbeatError if there is no file."""
        if not os.path.isfile(filepath):
            raise HeartbeatError("%s not found" % filepath)
        self.file_size = os.path.getsize(filepath)
        self.file_object = open(filepath, "rb")
        self.secret = secret
        self.challenges = []   # Challenge objects with their responses
        self._dev = None

    @classmethod
    def from_device(cls, ptr, length, secret=None):
        """A OneHash over `length` bytes at the device pointer `ptr`
        (hb_device_malloc): no file object; a call the GPU path does not take
        copies the bytes down once and answers from that copy."""
        self = cls.__new__(cls)
        self.file_size = int(length)
        self.file_object = None
        self.secret = secret
        self.challenges = []
        self._dev = int(ptr)
        return self

    def __del__(self):
        try:
            self.file_object.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ host path
    def _host_file(self):
        if self.file_object is None and self._dev is not None:
            buf = ctypes.create_string_buffer(max(1, self.file_size))
            ctx = multi.primary_context()
            with ctx.lock:
                if self.file_size:
                    ctx.check(_native.lib().hb_memcpy(ctx.h, buf, self._dev, self.file_size, 2))
            self.file_object = io.BytesIO(buf.raw[:self.file_size])
        return self.file_object

    def _host_meet(self, challenge):
        """One response by the reference's own file operations
        (OneHash.py:120-138): seek to the block; past file_size - chunk read
        the overhang first -- a read that stops at the end of the file -- and
        the rest of the chunk from the start; then the seed."""
        f = self._host_file()
        chunk = min(MAX_CHUNK, self.file_size // 10)
        block = challenge.block
        digest = hashlib.sha256()
        f.seek(block)
        last_start = self.file_size - chunk
        if block > last_start:
            over = block - last_start
            digest.update(f.read(over))
            f.seek(0)
            digest.update(f.read(chunk - over))
        else:
            digest.update(f.read(chunk))
        digest.update(challenge.seed)
        return digest.digest()

    def _gpu_takes(self, challenge):
        block, seed = challenge.block, challenge.seed
        return (isinstance(block, int) and 0 <= block < self.file_size and
                isinstance(seed, (bytes, bytearray)) and len(seed) <= MAX_GPU_SEED)

    def _leave_after(self, block):
        """Put the file object where the reference's reads leave it."""
        if self.file_object is None:
            return
        chunk = min(MAX_CHUNK, self.file_size // 10)
        last_start = self.file_size - chunk
        try:
            self.file_object.seek(block + chunk if block <= last_start else chunk - (block - last_start))
        except Exception:
            pass

    # ------------------------------------------------------------------ GPU path
    @staticmethod
    def _gpu_meet(pairs):
        """The responses of [(onehash, challenge), ...], all GPU-eligible, in
        one hb_onehash_meet_many call."""
        index, beats = {}, []
        for beat, _ in pairs:
            if id(beat) not in index:
                index[id(beat)] = len(beats)
                beats.append(beat)
        n = len(pairs)
        rec = np.zeros(n, dtype=_native.ONEHASH_JOB_DTYPE)
        rec["file"] = [index[id(beat)] for beat, _ in pairs]
        rec["block"] = [chal.block for _, chal in pairs]
        seeds = [bytes(chal.seed) for _, chal in pairs]
        lens = [len(s) for s in seeds]
        rec["seed_len"] = lens
        if lens and min(lens) == max(lens):
            if lens[0]:
                rec["seed"][:, :lens[0]] = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n, lens[0])
        else:
            for k, s in enumerate(seeds):
                rec["seed"][k, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        out = np.zeros(n * 32, dtype=np.uint8)
        srcs = _Sources(beats)
        with srcs as where:
            files = (_native.OneHashFile * len(beats))()
            for d, (addr, length) in zip(files, where):
                d.data, d.len = addr, length
            ctx = multi.primary_context()
            with ctx.lock:
                ctx.check(_native.lib().hb_onehash_meet_many(ctx.h, files, len(beats), rec.ctypes.data, n,
                                                             out.ctypes.data, srcs.flags))
        last = {}
        for beat, chal in pairs:
            last[id(beat)] = (beat, chal.block)
        for beat, block in last.values():
            beat._leave_after(block)
        raw = out.tobytes()
        return [raw[32 * k:32 * k + 32] for k in range(n)]

    @staticmethod
    def _gpu_generate(plan, chain=None):
        """plan: [(onehash, num, s0, secret bytes, blocks), ...] in one
        hb_onehash_generate_many call; fills every object's challenges.
        chain: "host" or "device" forces where the seed chains run."""
        beats = [p[0] for p in plan]
        total = sum(p[1] for p in plan)
        seeds = np.zeros(max(1, total) * 32, dtype=np.uint8)
        resp = np.zeros(max(1, total) * 32, dtype=np.uint8)
        srcs = _Sources(beats)
        with srcs as where:
            descs = (_native.OneHashGenDesc * len(plan))()
            keep = []
            for d, (addr, length), (_, num, s0, secret, blocks) in zip(descs, where, plan):
                arr = np.array(blocks, dtype=np.uint64)
                keep.append(arr)
                d.data, d.len, d.s0 = addr, length, s0
                d.secret, d.secret_len = secret, len(secret)
                d.num, d.blocks = num, (arr.ctypes.data if num else None)
            flags = srcs.flags | {None: 0, "host": _native.HB_ONEHASH_CHAIN_HOST,
                                  "device": _native.HB_ONEHASH_CHAIN_DEVICE}[chain]
            ctx = multi.primary_context()
            with ctx.lock:
                ctx.check(_native.lib().hb_onehash_generate_many(ctx.h, descs, len(plan), seeds.ctypes.data,
                                                                 resp.ctypes.data, flags))
        raw_s, raw_r = seeds.tobytes(), resp.tobytes()
        at = 0
        for beat, num, _, _, blocks in plan:
            made = []
            for k in range(num):
                lo = 32 * (at + k)
                chal = Challenge(blocks[k], raw_s[lo:lo + 32])
                chal.response = raw_r[lo:lo + 32]
                made.append(chal)
            at += num
            beat.challenges = made
            if num:
                beat._leave_after(blocks[-1])

    # ------------------------------------------------------------------ the reference's calls
    def generate_challenges(self, num, root_seed):
        """Replace ``challenges`` by `num` new ones: seed k of the chain from
        `root_seed`, block k of pick_blocks, and their response."""
        OneHash.generate_challenges_many([(self, num, root_seed)])

    @staticmethod
    def generate_challenges_many(items, chain=None):
        """generate_challenges for every item = (onehash, num, root_seed), the
        files of the batch in one GPU call.  Blocks are picked file by file in
        order, so the module-level generator ends where a loop of
        generate_challenges leaves it, and an item the reference fails on
        raises after the items before it are done, as a loop would."""
        plan, host, failure = [], [], None
        for beat, num, root_seed in items:
            try:
                s0 = OneHash._first_seed(num, root_seed, beat.secret)
                if not isinstance(num, int) or (num > 0 and not isinstance(beat.secret, (bytes, bytearray))):
                    # whatever range() makes of this num and hashlib of this secret (OneHash.py:162-165)
                    seeds = OneHash.generate_seeds(num, root_seed, beat.secret)
                    host.append((beat, seeds, beat.pick_blocks(num, root_seed)))
                    continue
                blocks = beat.pick_blocks(num, root_seed)
            except BaseException as e:
                failure = e
                break
            plan.append((beat, num, s0, bytes(beat.secret) if num else b"", blocks))
        if plan and _on_gpu(sum(p[1] for p in plan)):
            OneHash._gpu_generate(plan, chain)
        else:
            host = [(b, OneHash._chain(num, s0, secret), blocks)
                    for b, num, s0, secret, blocks in plan] + host
        for beat, seeds, blocks in host:
            made = []
            for block, seed in zip(blocks, seeds):
                chal = Challenge(block, seed)
                chal.response = beat._host_meet(chal)
                made.append(chal)
            beat.challenges = made
        if failure is not None:
            raise failure

    def meet_challenge(self, challenge):
        """SHA-256 of the challenged chunk and the seed.  The chunk is a tenth
        of the file, 1 KiB for files above 10 KiB; near the end of the file it
        wraps round to the start."""
        if self._gpu_takes(challenge) and _on_gpu(1):
            return OneHash._gpu_meet([(self, challenge)])[0]
        return self._host_meet(challenge)

    def meet_challenges(self, challenges):
        """[meet_challenge(c) for c in challenges] in one GPU call."""
        return OneHash.meet_many([(self, c) for c in challenges])

    @staticmethod
    def meet_many(pairs):
        """[onehash.meet_challenge(challenge) for onehash, challenge in pairs],
        whatever files the pairs name, in one GPU call."""
        pairs = list(pairs)
        out = [None] * len(pairs)
        gpu = [k for k, (beat, chal) in enumerate(pairs) if beat._gpu_takes(chal)]
        if not _on_gpu(len(gpu)):
            gpu = []
        taken = set(gpu)
        for k, (beat, chal) in enumerate(pairs):
            if k not in taken:
                out[k] = beat._host_meet(chal)
        if gpu:
            for k, r in zip(gpu, OneHash._gpu_meet([pairs[k] for k in gpu])):
                out[k] = r
        return out

    @staticmethod
    def _first_seed(num, root_seed, secret):
        """The checks of generate_seeds and the chain's first seed
        (OneHash.py:149-159)."""
        if num < 0:
            raise HeartbeatError('%s is not greater than 0' % num)
        if secret is None:
            raise HeartbeatError('secret can not be of type NoneType')
        try:
            return hashlib.sha256(root_seed).digest()
        except TypeError:
            return hashlib.sha256(str(root_seed).encode()).digest()

    @staticmethod
    def generate_seeds(num, root_seed, secret):
        """The `num` seeds of the chain from `root_seed`: SHA-256 of the root
        (of its str() if it is no bytes-like object), then each seed the
        SHA-256 of the one before followed by the secret.  Host code."""
        return OneHash._chain(num, OneHash._first_seed(num, root_seed, secret), secret)

    @staticmethod
    def _chain(num, seed, secret):
        seeds = []
        for _ in range(num):
            seeds.append(seed)
            link = hashlib.sha256(seed)
            link.update(secret)
            seed = link.digest()
        return seeds

    def pick_blocks(self, num, root_seed):
        """`num` positions inside the file, drawn from the module-level
        generator seeded with `root_seed` (OneHash.py:180-189)."""
        if num < 0:
            raise HeartbeatError('%s is not greater than 0' % num)
        random.seed(root_seed)
        top = self.file_size - 1
        picked = []
        for _ in range(num):
            picked.append(random.randint(0, top))
        return picked

    def check_answer(self, hash_answer):
        """True if `hash_answer` is the response of a stored challenge, which
        is then spent (an answer seen once could be replayed)."""
        if any(c.response == hash_answer for c in self.challenges):
            self.delete_challenge(hash_answer)
            return True
        return False

    def delete_challenge(self, hash_answer):
        """Drop the first stored challenge with this response; False if none."""
        for chal in self.challenges:
            if chal.response == hash_answer:
                self.challenges.remove(chal)
                return True
        return False

    def random_challenge(self):
        """A stored challenge picked by the module-level generator, without
        its answer."""
        return random.choice(self.challenges).without_answer

    @property
    def challenges_size(self):
        """sys.getsizeof of the challenge list."""
        return sys.getsizeof(self.challenges)


# the reference's module path (the repo's heartbeat/OneHash package re-exports these)
Challenge.__module__ = "heartbeat.OneHash.OneHash"
OneHash.__module__ = "heartbeat.OneHash.OneHash"
