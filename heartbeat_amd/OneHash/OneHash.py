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
what it is there.  ``pick_blocks_many`` and, with ``draw="device"``,
``generate_challenges_many`` draw the same positions on the GPU
(``hb_onehash_pick_blocks_many``, ``hb_onehash_generate_drawn_many``: CPython's
MT19937 bit for bit, a wave per file) for root seeds of type ``str``,
``bytes``, ``bytearray``, ``int`` and ``bool``, and set the generator to the
state the draws would have left; every other seed stays with ``pick_blocks``
(``HB_ONEHASH_DRAW_HOST=1`` / ``HB_ONEHASH_DRAW_DEVICE=1`` force either).

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
MAX_KEY_WORDS = _native.HB_ONEHASH_MAX_KEY_WORDS
# a generator state no random.seed() leaves (a seeded mt[0] is 0x80000000)
_UNSEEDED = (3, (0,) * 624 + (624,), None)


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


def _draw_forced():
    """"host", "device" or None, by HB_ONEHASH_DRAW_HOST / HB_ONEHASH_DRAW_DEVICE."""
    if os.environ.get("HB_ONEHASH_DRAW_HOST", "") not in ("", "0"):
        return "host"
    if os.environ.get("HB_ONEHASH_DRAW_DEVICE", "") not in ("", "0"):
        return "device"
    return None


def _draw_on_device(draw, jobs, files):
    """Are the positions of a GPU call of about `jobs` jobs over `files` files
    drawn on the device?  The caller's `draw`, then the two switches, then the
    forced path (HB_ONEHASH_DEVICE=1 includes the draw), then the library's
    choice: one file, from hb_onehash_draw_device_min_jobs() jobs."""
    if draw not in (None, "host", "device"):
        raise ValueError("draw is 'host', 'device' or None, not %r" % (draw,))
    mode = draw or _draw_forced()
    if mode is None and _forced() is not None:
        mode = _forced()
    if mode is not None:
        return mode == "device"
    if jobs <= 0 or files != 1:
        return False
    floor = _native.lib().hb_onehash_draw_device_min_jobs()
    return floor > 0 and jobs >= floor


def _draw_key(root_seed):
    """The key random.seed(root_seed) gives the generator (seed version 2), as
    little-endian 32-bit words, least significant first -- for a str, bytes or
    bytearray the seed followed by its SHA-512 read as one big-endian integer,
    for an int its absolute value -- or None for a seed the device draw does
    not take: another type (a subclass too), a str that does not encode, a key
    above HB_ONEHASH_MAX_KEY_WORDS words."""
    kind = type(root_seed)
    if kind in (int, bool):
        n = abs(int(root_seed))
    elif kind in (bytes, bytearray, str):
        try:
            a = root_seed.encode() if kind is str else bytes(root_seed)
        except UnicodeEncodeError:
            return None
        if len(a) + 64 > 4 * MAX_KEY_WORDS:
            return None
        n = int.from_bytes(a + hashlib.sha512(a).digest(), "big")
    else:
        return None
    words = max(1, (n.bit_length() + 31) // 32)
    if words > MAX_KEY_WORDS:
        return None
    return np.frombuffer(n.to_bytes(4 * words, "little"), dtype="<u4")


def _draw_takes(file_size, num, root_seed):
    """The key, if the device draws `num` positions of a file of `file_size`
    bytes under `root_seed`; None if pick_blocks does."""
    if not (isinstance(num, int) and 0 <= num <= 1 << 31 and isinstance(file_size, int)):
        return None
    if not ((1 if num else 0) <= file_size < 1 << 64):
        return None
    return _draw_key(root_seed)


def _host_pick(beat, num, root_seed, pending):
    """beat.pick_blocks(num, root_seed) while device draws may be pending.
    pending[0] is the pending draw that decides the generator's final state;
    it is cleared if this call reseeds the generator, which it may raise
    before doing.  While a draw is pending the generator's state is due to be
    replaced, so it is first set to one no seeding reaches and looked at
    afterwards."""
    if pending[0] is None:
        return beat.pick_blocks(num, root_seed)
    random.setstate(_UNSEEDED)
    try:
        return beat.pick_blocks(num, root_seed)
    finally:
        if random.getstate()[1] != _UNSEEDED[1]:
            pending[0] = None


def _set_generator(state_words):
    """Leave the module-level generator as random.seed and the draws left it:
    the 624 words and the index the device returned, no pending gauss value."""
    random.setstate((3, tuple(int(w) for w in state_words), None))


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
        An entry whose blocks are None goes on as (..., None, key, sets_state,
        root_seed): its positions are drawn on the device under `key`
        (_draw_key), in one hb_onehash_generate_drawn_many call for all such
        entries, and the one with sets_state leaves the module-level generator
        in its final state.
        chain: "host" or "device" forces where the seed chains run."""
        given = [p for p in plan if p[4] is not None]
        drawn = [p for p in plan if p[4] is None]
        made = {}
        if given:
            made.update(zip(map(id, given), OneHash._gpu_run(given, chain, False)))
        if drawn:
            made.update(zip(map(id, drawn), OneHash._gpu_run(drawn, chain, True)))
        for p in plan:   # in the caller's order: a file named twice keeps its last item's
            p[0].challenges = made[id(p)]
            if made[id(p)]:
                p[0]._leave_after(made[id(p)][-1].block)

    @staticmethod
    def _gpu_run(plan, chain, drawn):
        """One native call for plan entries of one kind (_gpu_generate); the
        Challenge list of every entry."""
        beats = [p[0] for p in plan]
        total = sum(p[1] for p in plan)
        seeds = np.zeros(max(1, total) * 32, dtype=np.uint8)
        resp = np.zeros(max(1, total) * 32, dtype=np.uint8)
        picked = np.zeros(max(1, total), dtype=np.uint64)
        state = np.zeros(_native.HB_ONEHASH_STATE_WORDS, dtype=np.uint32)
        srcs = _Sources(beats)
        with srcs as where:
            descs = ((_native.OneHashDrawnDesc if drawn else _native.OneHashGenDesc) * len(plan))()
            keep, at = [], 0
            for d, (addr, length), p in zip(descs, where, plan):
                num, s0, secret = p[1:4]
                d.data, d.len, d.s0 = addr, length, s0
                d.secret, d.secret_len = secret, len(secret)
                d.num = num
                if drawn:
                    d.key, d.key_words = p[5].ctypes.data, len(p[5])
                    d.blocks_out = picked.ctypes.data + 8 * at if num else None
                    d.state_out = state.ctypes.data if p[6] else None
                else:
                    arr = np.array(p[4], dtype=np.uint64)
                    keep.append(arr)
                    d.blocks = arr.ctypes.data if num else None
                at += num
            flags = srcs.flags | {None: 0, "host": _native.HB_ONEHASH_CHAIN_HOST,
                                  "device": _native.HB_ONEHASH_CHAIN_DEVICE}[chain]
            call = _native.lib().hb_onehash_generate_drawn_many if drawn else _native.lib().hb_onehash_generate_many
            ctx = multi.primary_context()
            with ctx.lock:
                ctx.check(call(ctx.h, descs, len(plan), seeds.ctypes.data, resp.ctypes.data, flags))
        if drawn:
            if any(p[6] for p in plan):
                _set_generator(state)
            at, flat = 0, picked.tolist()
            plan, entries = [], plan
            for p in entries:
                plan.append(p[:4] + (flat[at:at + p[1]],))
                at += p[1]
        raw_s, raw_r = seeds.tobytes(), resp.tobytes()
        at, out = 0, []
        for _, num, _, _, blocks in plan:
            made = []
            for k in range(num):
                lo = 32 * (at + k)
                chal = Challenge(blocks[k], raw_s[lo:lo + 32])
                chal.response = raw_r[lo:lo + 32]
                made.append(chal)
            at += num
            out.append(made)
        return out

    # ------------------------------------------------------------------ the reference's calls
    def generate_challenges(self, num, root_seed):
        """Replace ``challenges`` by `num` new ones: seed k of the chain from
        `root_seed`, block k of pick_blocks, and their response."""
        OneHash.generate_challenges_many([(self, num, root_seed)])

    @staticmethod
    def generate_challenges_many(items, chain=None, draw=None):
        """generate_challenges for every item = (onehash, num, root_seed), the
        files of the batch in one GPU call.  Blocks are those of pick_blocks
        file by file in order, the module-level generator ends where a loop of
        generate_challenges leaves it, and an item the reference fails on
        raises after the items before it are done, as a loop would.

        draw: "device" has the GPU call draw the positions too, for the items
        it takes (_draw_takes) -- the generator is then set to the state the
        last item that seeded it leaves, whichever side drew that one; "host"
        keeps every draw on pick_blocks; None follows HB_ONEHASH_DRAW_HOST /
        HB_ONEHASH_DRAW_DEVICE, then HB_ONEHASH_DEVICE, then the measured
        default: a call of one file from hb_onehash_draw_device_min_jobs()
        jobs draws on the device, a call of several files on the host."""
        items = list(items)
        on_device = _draw_on_device(draw, sum(it[1] for it in items if isinstance(it[1], int) and it[1] > 0),
                                    len(items))
        plan, host, failure = [], [], None
        pending = [None]   # the plan entry whose device draw decides the generator's state so far
        for beat, num, root_seed in items:
            try:
                s0 = OneHash._first_seed(num, root_seed, beat.secret)
                if not isinstance(num, int) or (num > 0 and not isinstance(beat.secret, (bytes, bytearray))):
                    # whatever range() makes of this num and hashlib of this secret (OneHash.py:162-165)
                    seeds = OneHash.generate_seeds(num, root_seed, beat.secret)
                    host.append((beat, seeds, _host_pick(beat, num, root_seed, pending)))
                    continue
                key = _draw_takes(beat.file_size, num, root_seed) if on_device else None
                blocks = _host_pick(beat, num, root_seed, pending) if key is None else None
            except BaseException as e:
                failure = e
                break
            if key is None:
                plan.append((beat, num, s0, bytes(beat.secret) if num else b"", blocks))
            else:
                pending[0] = len(plan)
                plan.append((beat, num, s0, bytes(beat.secret) if num else b"", None, key, False, root_seed))
        if plan and _on_gpu(sum(p[1] for p in plan)):
            if pending[0] is not None:
                p = plan[pending[0]]
                plan[pending[0]] = p[:6] + (True,) + p[7:]
            OneHash._gpu_generate(plan, chain)
        else:
            if any(p[4] is None for p in plan):
                # no GPU call after all: the pending draws, in order, by pick_blocks
                left = random.getstate()
                plan = [p if p[4] is not None else p[:4] + (p[0].pick_blocks(p[1], p[7]),) for p in plan]
                if pending[0] is None:
                    random.setstate(left)
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

    @staticmethod
    def pick_blocks_many(items):
        """[pick_blocks(num, root_seed) for every item = (onehash or file
        size, num, root_seed)], the draws in one GPU launch
        (hb_onehash_pick_blocks_many), and the module-level generator left
        where that loop leaves it: in the state of the last item that seeded
        it.  Items the device draw does not take (_draw_takes) are drawn by
        pick_blocks itself, in order, so an item it fails on raises as in the
        loop, after the items before it.  HB_ONEHASH_HOST=1 or
        HB_ONEHASH_DRAW_HOST=1 keep every draw on pick_blocks."""
        def sized(file_size):
            beat = OneHash.__new__(OneHash)   # pick_blocks reads the size alone
            beat.file_size, beat.file_object, beat._dev = file_size, None, None
            return beat

        items = [(x if isinstance(x, OneHash) else sized(x), num, root) for x, num, root in items]
        on_device = _forced() != "host" and _draw_forced() != "host"
        out, drawn, failure = [None] * len(items), [], None
        pending = [None]
        for k, (beat, num, root_seed) in enumerate(items):
            key = _draw_takes(beat.file_size, num, root_seed) if on_device else None
            if key is None:
                try:
                    out[k] = _host_pick(beat, num, root_seed, pending)
                except BaseException as e:
                    failure = e
                    break
            else:
                pending[0] = len(drawn)
                drawn.append((k, beat.file_size, num, key))
        if drawn:
            total = sum(d[2] for d in drawn)
            picked = np.zeros(max(1, total), dtype=np.uint64)
            state = np.zeros(_native.HB_ONEHASH_STATE_WORDS, dtype=np.uint32)
            descs = (_native.OneHashDrawDesc * len(drawn))()
            at = 0
            for j, (d, (_, size, num, key)) in enumerate(zip(descs, drawn)):
                d.len, d.key, d.key_words, d.num = size, key.ctypes.data, len(key), num
                d.blocks_out = picked.ctypes.data + 8 * at if num else None
                d.state_out = state.ctypes.data if j == pending[0] else None
                at += num
            ctx = multi.primary_context()
            with ctx.lock:
                ctx.check(_native.lib().hb_onehash_pick_blocks_many(ctx.h, descs, len(drawn), 0))
            if pending[0] is not None:
                _set_generator(state)
            at, flat = 0, picked.tolist()
            for k, _, num, _ in drawn:
                out[k] = flat[at:at + num]
                at += num
        if failure is not None:
            raise failure
        return out

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
