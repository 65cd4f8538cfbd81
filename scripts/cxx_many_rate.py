"""Batched cxx encode against a loop of single cxx encodes: per
shape, after a warm-up of both, 7 alternating rounds of

  A: a loop of hb_encode(HB_PRF_CXX) calls, one per file (the parent's path);
  B: one hb_cxx_encode_many over the same files;

each timed with a host clock around calls that return after a stream
synchronise.  Prints the minimum and the spread (max - min) of both arms and
B's slowest round against A's fastest.  B's tags and tries are compared with
A's on every shape before any timing.  Shapes run device-resident ("dev") or
from host memory ("host"); "api" is heartbeat.Heartbeat().encode_many over
BytesIO files against a loop of encode().

  python scripts/cxx_many_rate.py [--rounds 7] [--out FILE] [SHAPE ...]
  SHAPE = bits:S:files:bytes:dev|host (bits "P256": the benchmark's prime) or "api"
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
DEFAULT = ["1024:10:256:%d:dev" % MIB, "1024:10:256:%d:host" % MIB, "P256:16:4096:65536:dev",
           "P256:16:4096:65536:host"]
DEFAULT += ["1024:10:%d:%d:%s" % (n, MIB, where) for n in (16, 4, 3, 2, 1) for where in ("dev", "host")]
DEFAULT += ["api"]
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
           "B_slowest_beats_A_fastest": max(b) < min(a), "B_no_slower": min(b) <= min(a)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def encode_shape(bits, S, nfiles, size, where, rounds):
    p = prime(bits)
    w = nat.width_of(p)
    C = (p.bit_length() // 8) * S
    nb = size // C + 1
    ctx = nat.context()
    L = nat.lib()
    dev = where == "dev"
    flags = 3 if dev else 0
    tstride = (nb * w + 15) // 16 * 16
    bufs = []
    if dev:
        d, ta, tb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        for x, n in ((d, nfiles * size), (ta, nfiles * tstride), (tb, nfiles * tstride)):
            ctx.check(L.hb_device_malloc(ctx.h, n, ctypes.byref(x)))
            bufs.append(x)
        ctx.check(L.hb_fill_random(ctx.h, d, nfiles * size, 4242))
        d, ta, tb = d.value, ta.value, tb.value
    else:
        hd = np.random.default_rng(4242).integers(0, 256, nfiles * size, dtype=np.uint8)
        ha, hb = np.zeros(nfiles * tstride, dtype=np.uint8), np.zeros(nfiles * tstride, dtype=np.uint8)
        d, ta, tb = hd.ctypes.data, ha.ctypes.data, hb.ctypes.data
    keys = [(hashlib.sha256(b"f%d" % i).digest(), hashlib.sha256(b"a%d" % i).digest()) for i in range(nfiles)]
    pb = nat.be(p)
    ctx.prepare(p.bit_length())
    descs = (nat.FileDesc * nfiles)()
    for i in range(nfiles):
        descs[i].f_key, descs[i].alpha_key = keys[i]
        descs[i].data = d + i * size
        descs[i].len = size
        descs[i].tags = tb + i * tstride
    tries_a, tries_b = ctypes.c_uint64(), ctypes.c_uint64()

    def arm_a():
        total = 0
        t0 = time.perf_counter()
        for i in range(nfiles):
            ctx.check(L.hb_encode(ctx.h, pb, len(pb), S, keys[i][0], keys[i][1], 32, 0, d + i * size, size,
                                  nb, ta + i * tstride, flags | nat.HB_PRF_CXX, ctypes.byref(tries_a)))
            total += tries_a.value
        return time.perf_counter() - t0, total

    def arm_b():
        t0 = time.perf_counter()
        ctx.check(L.hb_cxx_encode_many(ctx.h, pb, len(pb), S, 32, descs, nfiles, flags, ctypes.byref(tries_b)))
        return time.perf_counter() - t0, tries_b.value

    try:
        _, na = arm_a()   # warm-up, and the tags to compare
        _, nb_tries = arm_b()
        if dev:
            ha, hb = np.empty(nfiles * tstride, dtype=np.uint8), np.empty(nfiles * tstride, dtype=np.uint8)
            ctx.check(L.hb_memcpy(ctx.h, ha.ctypes.data, ta, len(ha), 2))
            ctx.check(L.hb_memcpy(ctx.h, hb.ctypes.data, tb, len(hb), 2))
        equal = all(bytes(ha[i * tstride:i * tstride + nb * w]) == bytes(hb[i * tstride:i * tstride + nb * w])
                    for i in range(nfiles))
        if not equal or na != nb_tries:
            raise SystemExit("batched tags or tries differ from the loop's (%s, %d vs %d tries)" % (equal, na, nb_tries))
        a, b = [], []
        for _ in range(rounds):
            a.append(arm_a()[0])
            b.append(arm_b()[0])
        launches = ctx.last_kernel_ms()[1]
    finally:
        for x in bufs:
            ctx.check(L.hb_device_free(ctx.h, x))
    gib = nfiles * size / float(1 << 30)
    return report("encode %s-bit S=%d, %d x %d bytes (%s)" % (bits, S, nfiles, size, where), a, b,
                  {"tags_equal": equal, "blocks_per_file": nb, "B_launches": launches,
                   "A_gib_s": round(gib / min(a), 2), "B_gib_s": round(gib / min(b), 2)})


def api_shape(rounds, nfiles=256, size=MIB):
    import heartbeat
    rng = np.random.default_rng(11)
    blobs = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(nfiles)]
    beat = heartbeat.Heartbeat(prime=prime(1024))
    pub = beat.get_public()

    def arm_a():
        t0 = time.perf_counter()
        res = [beat.encode(io.BytesIO(x)) for x in blobs]
        return time.perf_counter() - t0, res

    def arm_b():
        t0 = time.perf_counter()
        res = beat.encode_many([io.BytesIO(x) for x in blobs])
        return time.perf_counter() - t0, res

    arm_a()
    _, res = arm_b()
    # fresh keys per call: the batch's tags are checked by a proof instead
    ok = True
    for i in (0, nfiles // 2, nfiles - 1):
        tag, state = res[i]
        chal = beat.gen_challenge(state)
        ok = ok and beat.verify(pub.prove(io.BytesIO(blobs[i]), chal, tag), chal, state) is True
    if not ok:
        raise SystemExit("a batched tag does not verify")
    a, b = [], []
    for _ in range(rounds):
        a.append(arm_a()[0])
        b.append(arm_b()[0])
    return report("encode 1024-bit S=10, %d x %d bytes BytesIO (Heartbeat.encode_many vs encode loop)" % (nfiles, size),
                  a, b, {"proofs_verify": ok})


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
            bits, S, n, size, where = s.split(":")
            rows.append(encode_shape(bits if bits == "P256" else int(bits), int(S), int(n), int(size), where, rounds))
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
