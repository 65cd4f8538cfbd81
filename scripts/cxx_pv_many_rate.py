"""Batched cxx prove and verify against loops of the single calls (DESIGN.md
5.3e): per shape, after a warm-up of both, 7 alternating rounds of

  A: a loop of hb_prove(HB_PRF_CXX) resp. hb_cxx_verify_rhs calls, one per
     proof (the single calls, which the batch leaves as they were);
  B: one hb_cxx_prove_many resp. hb_cxx_verify_rhs_many over the same proofs;

each timed with a host clock around calls that return after a stream
synchronise.  Prints the minimum and the spread (max - min) of both arms and
B's slowest round against A's fastest.  B's results are compared with A's on
every shape before any timing.  The challenge is check_fraction of the file's
blocks: 1.0 is the cxx default (check_all, every block in order), 0.3 a sampled
one.  Prove shapes run device-resident ("dev") or from host memory ("host");
"api" is heartbeat.Heartbeat().prove_many / verify_many over BytesIO files
against loops of prove() / verify().

  python scripts/cxx_pv_many_rate.py [--rounds 7] [--out FILE] [SHAPE ...]
  SHAPE = prove:bits:S:proofs:bytes:fraction:dev|host | verify:bits:S:proofs:bytes:fraction | api
  (bits "P256": the benchmark's prime)
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
COUNTS = (256, 16, 4, 3, 2, 1)
DEFAULT = ["prove:1024:10:%d:%d:%s:%s" % (n, MIB, f, where) for f in ("1.0", "0.3") for where in ("dev", "host")
           for n in COUNTS]
DEFAULT += ["verify:1024:10:%d:%d:%s" % (n, MIB, f) for f in ("1.0", "0.3") for n in COUNTS]
DEFAULT += ["prove:P256:16:256:%d:1.0:dev" % MIB, "prove:P256:16:256:%d:1.0:host" % MIB, "verify:P256:16:256:%d:1.0" % MIB]
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


def rounds_of(arm_a, arm_b, rounds):
    ra, rb = arm_a()[1], arm_b()[1]   # warm-up, and the results to compare
    if ra != rb:
        raise SystemExit("the batch's results differ from the loop's")
    a, b = [], []
    for _ in range(rounds):
        a.append(arm_a()[0])
        b.append(arm_b()[0])
    return a, b


def prove_shape(bits, S, n, size, fraction, where, rounds):
    p = prime(bits)
    w = nat.width_of(p)
    C = (p.bit_length() // 8) * S
    ntags = size // C + 1
    chunks = int(fraction * ntags)
    ctx = nat.context()
    L = nat.lib()
    dev = where == "dev"
    flags = 3 if dev else 0
    tstride = (ntags * w + 15) // 16 * 16
    bufs = []
    if dev:
        d, t = ctypes.c_void_p(), ctypes.c_void_p()
        for x, m, seed in ((d, n * size, 4242), (t, n * tstride, 4243)):
            ctx.check(L.hb_device_malloc(ctx.h, m, ctypes.byref(x)))
            bufs.append(x)
            ctx.check(L.hb_fill_random(ctx.h, x, m, seed))   # a prove takes any tag values
        d, t = d.value, t.value
    else:
        rng = np.random.default_rng(4242)
        hd, ht = rng.integers(0, 256, n * size, dtype=np.uint8), rng.integers(0, 256, n * tstride, dtype=np.uint8)
        d, t = hd.ctypes.data, ht.ctypes.data
    keys = [hashlib.sha256(b"c%d" % i).digest() for i in range(n)]
    pb = nat.be(p)
    ctx.prepare(p.bit_length())
    out_a, out_b = ctypes.create_string_buffer(n * (S + 1) * w), ctypes.create_string_buffer(n * (S + 1) * w)
    base = ctypes.addressof(out_b)
    descs = (nat.ProveDesc * n)()
    for i in range(n):
        e = descs[i]
        e.chal_key, e.chunks = keys[i], chunks
        e.vmax_be, e.vmax_len = pb, len(pb)
        e.tags, e.ntags = t + i * tstride, ntags
        e.data, e.len = d + i * size, size
        e.mu_out, e.sigma_out = base + i * (S + 1) * w, base + (i * (S + 1) + S) * w

    def arm_a():
        a0 = ctypes.addressof(out_a)
        t0 = time.perf_counter()
        for i in range(n):
            ctx.check(L.hb_prove(ctx.h, pb, len(pb), S, keys[i], 32, chunks, pb, len(pb), t + i * tstride, ntags,
                                 d + i * size, size, flags | nat.HB_PRF_CXX, a0 + i * (S + 1) * w,
                                 a0 + (i * (S + 1) + S) * w))
        return time.perf_counter() - t0, out_a.raw

    def arm_b():
        t0 = time.perf_counter()
        ctx.check(L.hb_cxx_prove_many(ctx.h, pb, len(pb), S, 32, descs, n, flags))
        return time.perf_counter() - t0, out_b.raw

    try:
        a, b = rounds_of(arm_a, arm_b, rounds)
        launches = ctx.last_kernel_ms()[1]
    finally:
        for x in bufs:
            ctx.check(L.hb_device_free(ctx.h, x))
    return report("prove %s-bit S=%d, %d x %d bytes, fraction %s: %d of %d chunks (%s)" % (
        bits, S, n, size, fraction, min(chunks, ntags), ntags, where), a, b,
        {"results_equal": True, "B_launches": launches, "A_ms_per_proof": round(min(a) * 1e3 / n, 4),
         "B_ms_per_proof": round(min(b) * 1e3 / n, 4)})


def verify_shape(bits, S, n, size, fraction, rounds):
    p = prime(bits)
    w = nat.width_of(p)
    C = (p.bit_length() // 8) * S
    nstate = size // C + 1
    chunks = int(fraction * nstate)
    ctx = nat.context()
    L = nat.lib()
    rng = random.Random(77)
    keys = [tuple(hashlib.sha256(b"%s%d" % (c, i)).digest() for c in (b"f", b"a", b"c")) for i in range(n)]
    mus = [b"".join(rng.randrange(p).to_bytes(w, "big") for _ in range(S)) for _ in range(n)]
    pb = nat.be(p)
    ctx.prepare(p.bit_length())
    out_a, out_b = ctypes.create_string_buffer(n * w), ctypes.create_string_buffer(n * w)
    descs = (nat.VerifyDesc * n)()
    for i in range(n):
        e = descs[i]
        e.f_key, e.alpha_key, e.chal_key = keys[i]
        e.state_chunks, e.chunks = nstate, chunks
        e.vmax_be, e.vmax_len = pb, len(pb)
        e.mu = mus[i]
        e.rhs_out = ctypes.addressof(out_b) + i * w

    def arm_a():
        a0 = ctypes.addressof(out_a)
        t0 = time.perf_counter()
        for i in range(n):
            fk, ak, ck = keys[i]
            ctx.check(L.hb_cxx_verify_rhs(ctx.h, pb, len(pb), S, fk, ak, 32, nstate, ck, 32, chunks, pb, len(pb),
                                          mus[i], a0 + i * w))
        return time.perf_counter() - t0, out_a.raw

    def arm_b():
        t0 = time.perf_counter()
        ctx.check(L.hb_cxx_verify_rhs_many(ctx.h, pb, len(pb), S, 32, 32, descs, n, 0))
        return time.perf_counter() - t0, out_b.raw

    a, b = rounds_of(arm_a, arm_b, rounds)
    return report("verify %s-bit S=%d, %d proofs of %d-byte files, fraction %s: %d of %d chunks" % (
        bits, S, n, size, fraction, min(chunks, nstate), nstate), a, b,
        {"results_equal": True, "B_launches": ctx.last_kernel_ms()[1], "A_ms_per_proof": round(min(a) * 1e3 / n, 4),
         "B_ms_per_proof": round(min(b) * 1e3 / n, 4)})


def api_shapes(rounds, n=256, size=MIB):
    import heartbeat
    rng = np.random.default_rng(11)
    blobs = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(n)]
    beat = heartbeat.Heartbeat(prime=prime(1024))
    pub = beat.get_public()
    enc = beat.encode_many([io.BytesIO(x) for x in blobs])
    rows = []
    for fraction in (1.0, 0.3):
        beat.check_fraction = fraction
        chals = [beat.gen_challenge(state) for _, state in enc]

        def prove_a():
            t0 = time.perf_counter()
            res = [pub.prove(io.BytesIO(x), c, tag) for x, c, (tag, _) in zip(blobs, chals, enc)]
            return time.perf_counter() - t0, [(q.mu, q.sigma) for q in res]

        def prove_b():
            t0 = time.perf_counter()
            res = pub.prove_many([(io.BytesIO(x), c, tag) for x, c, (tag, _) in zip(blobs, chals, enc)])
            return time.perf_counter() - t0, [(q.mu, q.sigma) for q in res]

        a, b = rounds_of(prove_a, prove_b, rounds)
        rows.append(report("Heartbeat().prove_many vs prove loop, 1024-bit S=10, %d x %d bytes BytesIO, "
                           "check_fraction %s" % (n, size, fraction), a, b, {"results_equal": True}))
        proofs = pub.prove_many([(io.BytesIO(x), c, tag) for x, c, (tag, _) in zip(blobs, chals, enc)])
        items = [(q, c, state) for q, c, (_, state) in zip(proofs, chals, enc)]

        def verify_a():
            t0 = time.perf_counter()
            res = [beat.verify(*it) for it in items]
            return time.perf_counter() - t0, res

        def verify_b():
            t0 = time.perf_counter()
            res = beat.verify_many(items)
            return time.perf_counter() - t0, res

        if verify_b()[1] != [True] * n:
            raise SystemExit("a batched proof does not verify")
        a, b = rounds_of(verify_a, verify_b, rounds)
        rows.append(report("Heartbeat().verify_many vs verify loop, 1024-bit S=10, %d proofs, check_fraction %s" % (
            n, fraction), a, b, {"results_equal": True, "all_verify": True}))
    return rows


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
        f = s.split(":")
        bits = f[1] if len(f) > 1 and f[1] == "P256" else int(f[1]) if len(f) > 1 else None
        if s == "api":
            rows += api_shapes(rounds)
        elif f[0] == "prove":
            rows.append(prove_shape(bits, int(f[2]), int(f[3]), int(f[4]), float(f[5]), f[6], rounds))
        else:
            rows.append(verify_shape(bits, int(f[2]), int(f[3]), int(f[4]), float(f[5]), rounds))
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
