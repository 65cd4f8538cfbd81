"""Batched prove against a loop of single proves: per shape,
after a warm-up of both, 7 alternating rounds of

  A: a loop of hb_prove calls, one per proof;
  B: one hb_prove_many over the same proofs;

each timed with a host clock around calls that return after the stream is
synchronised (mu and sigma into host buffers).  Files and tags are either
device-resident (HB_DATA_ON_DEVICE | HB_TAGS_ON_DEVICE, 16-byte aligned, as a
storage node that keeps its shards on the GPU holds them; "devodd": at odd
addresses, which keeps the batch's sums on byte loads) or in host memory.
Prints the minimum and the spread (max - min) of both arms and B's slowest
round against A's fastest.  B's mu and sigma are compared with A's before any
timing.  The "api" shape goes through the Python API: PySwizzle.prove_many
against a loop of PySwizzle.prove over BytesIO files.

  python scripts/prove_many_rate.py [--rounds 7] [--out FILE] [SHAPE ...]
  SHAPE = bits:S:proofs:chunks:file bytes:dev|devodd|host (bits "P256": the
          benchmark's prime) or "api"
"""
import ctypes
import hashlib
import io
import json
import random
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402

MIB = 1 << 20
DEFAULT = ["1024:10:256:820:%d:dev" % MIB, "1024:10:256:820:%d:host" % MIB, "P256:16:4096:129:65536:dev",
           "P256:16:4096:129:65536:host", "P256:16:256:10000:%d:dev" % (3 * MIB),
           "1024:10:256:820:%d:devodd" % MIB, "P256:16:4096:129:65536:devodd"] + \
          ["1024:10:%d:820:%d:%s" % (n, MIB, where) for n in (16, 4, 3, 2, 1) for where in ("dev", "host")] + ["api"]
P256 = int("db8709c32591ddc589b5c3c0986f92e0d11205b943c23a7e419e6c35b0256e6b", 16)


def prime(bits):
    if bits == "P256":
        return P256
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["_is_probable_prime"])
    rng = random.Random(5000 + int(bits))
    while True:
        x = rng.getrandbits(int(bits)) | (1 << (int(bits) - 1)) | 1
        if pys._is_probable_prime(x):
            return x


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
            "spread_ms": round((max(ts) - min(ts)) * 1e3, 3)}


def report(shape, a, b, extra):
    row = {"shape": shape, "A_loop": stats(a), "B_batch": stats(b),
           "ratio_minA_over_maxB": round(min(a) / max(b), 2), "ratio_min_over_min": round(min(a) / min(b), 2),
           "B_slowest_beats_A_fastest": max(b) < min(a)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def key_of(i):
    return hashlib.sha256(b"c/%d" % i).digest()


class Dev(object):
    """One device allocation filled with seeded bytes (hb_fill_random)."""

    def __init__(self, ctx, n, seed):
        self.ctx, self.n = ctx, n
        p = ctypes.c_void_p()
        ctx.check(nat.lib().hb_device_malloc(ctx.h, n, ctypes.byref(p)))
        self.p = p.value
        ctx.check(nat.lib().hb_fill_random(ctx.h, self.p, n, seed))

    def download(self):
        out = np.empty(self.n, dtype=np.uint8)
        self.ctx.check(nat.lib().hb_memcpy(self.ctx.h, out.ctypes.data, self.p, self.n, 2))
        return out

    def free(self):
        self.ctx.check(nat.lib().hb_device_free(self.ctx.h, self.p))


def abi_shape(bits, S, nproofs, chunks, length, where, rounds):
    p = prime(bits)
    w = nat.width_of(p)
    C = (p.bit_length() // 8) * S
    ntags = length // C + 1
    ctx = nat.context()
    L = nat.lib()
    pb = nat.be(p)
    ctx.prepare(p.bit_length())
    odd = 1 if where == "devodd" else 0
    dstride, tstride = ((length + 15) & ~15) + 2 * odd, ((ntags * w + 15) & ~15) + 2 * odd
    # seeded bytes for every file and tag array (tags are the caller's bytes:
    # any value of the tag width), made on the device and copied to the host
    # for the host shapes
    ddev, tdev = Dev(ctx, dstride * nproofs + 16, 0x5EED0100), Dev(ctx, tstride * nproofs + 16, 0x5EED0200)
    try:
        flags = 0 if where == "host" else 3
        if flags:
            dbase, tbase = ddev.p + odd, tdev.p + odd
        else:
            dhost, thost = ddev.download(), tdev.download()
            dbase, tbase = dhost.ctypes.data, thost.ctypes.data
        ra = ctypes.create_string_buffer(nproofs * (S + 1) * w)
        rb = ctypes.create_string_buffer(nproofs * (S + 1) * w)
        keys = [key_of(i) for i in range(nproofs)]
        descs = (nat.ProveDesc * nproofs)()
        for i in range(nproofs):
            d = descs[i]
            d.chal_key, d.chunks = keys[i], chunks
            d.vmax_be, d.vmax_len = pb, len(pb)
            d.tags, d.ntags = tbase + i * tstride, ntags
            d.data, d.len = dbase + i * dstride, length
            d.mu_out = ctypes.addressof(rb) + i * (S + 1) * w
            d.sigma_out = ctypes.addressof(rb) + (i * (S + 1) + S) * w
        a0 = ctypes.addressof(ra)

        def arm_a():
            t0 = time.perf_counter()
            for i in range(nproofs):
                ctx.check(L.hb_prove(ctx.h, pb, len(pb), S, keys[i], 32, chunks, pb, len(pb), tbase + i * tstride, ntags,
                                     dbase + i * dstride, length, flags, a0 + i * (S + 1) * w,
                                     a0 + (i * (S + 1) + S) * w))
            return time.perf_counter() - t0

        def arm_b():
            t0 = time.perf_counter()
            ctx.check(L.hb_prove_many(ctx.h, pb, len(pb), S, 32, descs, nproofs, flags))
            return time.perf_counter() - t0

        arm_a()   # warm-up, and the results to compare
        arm_b()
        n1 = (S + 1) * w
        equal = ra.raw == rb.raw and len(set(ra.raw[i * n1:(i + 1) * n1] for i in range(nproofs))) == nproofs
        if not equal:
            raise SystemExit("the batch's proofs differ from the loop's")
        a, b = [], []
        for _ in range(rounds):
            a.append(arm_a())
            b.append(arm_b())
    finally:
        ddev.free()
        tdev.free()
    return report("%s-bit S=%d, %d proofs x %d chunks, %d-byte files, %s" % (bits, S, nproofs, chunks, length, where),
                  a, b, {"proofs_equal": equal, "A_us_per_proof": round(min(a) / nproofs * 1e6, 1),
                         "B_us_per_proof": round(min(b) / nproofs * 1e6, 1)})


def api_shape(rounds, bits=1024, S=10, nproofs=256, chunks=820, length=MIB):
    from heartbeat_amd.PySwizzle import PySwizzle
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["Tag"])
    p = prime(bits)
    w = nat.width_of(p)
    ntags = length // ((p.bit_length() // 8) * S) + 1
    beat = PySwizzle(S, b"k" * 32, p)
    rng = np.random.default_rng(0x5EED)
    items = []
    for i in range(nproofs):
        data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        tag = pys.Tag._from_raw(memoryview(rng.integers(0, 256, ntags * w, dtype=np.uint8)), w)
        items.append((io.BytesIO(data), pys.Challenge(chunks, p, key_of(i)), tag))

    def arm_a():
        t0 = time.perf_counter()
        res = [beat.prove(*it) for it in items]
        return time.perf_counter() - t0, res

    def arm_b():
        t0 = time.perf_counter()
        res = beat.prove_many(items)
        return time.perf_counter() - t0, res

    _, wa = arm_a()
    _, wb = arm_b()
    equal = [(x.mu, x.sigma) for x in wa] == [(x.mu, x.sigma) for x in wb] and len({x.sigma for x in wa}) == nproofs
    if not equal:
        raise SystemExit("prove_many differs from the loop of prove")
    a, b = [], []
    for _ in range(rounds):
        a.append(arm_a()[0])
        b.append(arm_b()[0])
    return report("%d-bit S=%d, %d proofs x %d chunks, %d-byte files (PySwizzle.prove_many vs prove loop)" % (
        bits, S, nproofs, chunks, length), a, b, {"results_equal": equal})


def main(argv):
    rounds, out, shapes = 7, None, []
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        else:
            shapes.append(x)
    rows = []
    for s in shapes or DEFAULT:
        if s == "api":
            rows.append(api_shape(rounds))
        else:
            bits, S, n, chunks, length, where = s.split(":")
            rows.append(abi_shape(bits if bits == "P256" else int(bits), int(S), int(n), int(chunks), int(length),
                                  where, rounds))
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
