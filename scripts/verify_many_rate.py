"""Batched verify against a loop of single verifies: per shape,
after a warm-up of both, 7 alternating rounds of

  A: a loop of hb_verify_rhs calls, one per proof;
  B: one hb_verify_rhs_many over the same proofs;

each timed with a host clock around calls that return after the stream is
synchronised (host buffers in, host buffers out, as an auditor holds them).
Prints the minimum and the spread (max - min) of both arms and B's slowest
round against A's fastest.  B's right-hand sides are compared with A's before
any timing.  The "api" shape goes through the Python API:
PySwizzle.verify_many against a loop of PySwizzle.verify.

  python scripts/verify_many_rate.py [--rounds 7] [--out FILE] [SHAPE ...]
  SHAPE = bits:S:proofs:chunks (bits "P256": the benchmark's prime) or "api"
"""
import ctypes
import hashlib
import json
import random
import sys
import time

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402

DEFAULT = ["1024:10:256:820", "P256:16:4096:129", "P256:16:256:10000", "1024:10:1:820", "1024:10:4:820",
           "1024:10:16:820", "api"]
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


def h(tag, i, n):
    out = b""
    k = 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d/%d" % (tag, i, k)).digest()
        k += 1
    return out[:n]


def proofs_of(p, S, nproofs, chunks):
    """Seeded (f_key, alpha_key, chal_key, mu bytes) per proof; state_chunks =
    chunks and v_max = p, PySwizzle.gen_challenge's choice."""
    w = nat.width_of(p)
    out = []
    for i in range(nproofs):
        mu = b"".join((int.from_bytes(h(b"mu%d" % j, i, w), "big") % p).to_bytes(w, "big") for j in range(S))
        out.append((h(b"f", i, 32), h(b"a", i, 32), h(b"c", i, 32), mu))
    return out


def abi_shape(bits, S, nproofs, chunks, rounds):
    p = prime(bits)
    w = nat.width_of(p)
    ctx = nat.context()
    L = nat.lib()
    pb = nat.be(p)
    ctx.prepare(p.bit_length())
    items = proofs_of(p, S, nproofs, chunks)
    ra = ctypes.create_string_buffer(nproofs * w)
    rb = ctypes.create_string_buffer(nproofs * w)
    rhs1 = [ctypes.addressof(ra) + i * w for i in range(nproofs)]
    descs = (nat.VerifyDesc * nproofs)()
    for i, (fk, ak, ck, mu) in enumerate(items):
        d = descs[i]
        d.f_key, d.alpha_key, d.chal_key = fk, ak, ck
        d.state_chunks, d.chunks = chunks, chunks
        d.vmax_be, d.vmax_len = pb, len(pb)
        d.mu = mu
        d.rhs_out = ctypes.addressof(rb) + i * w

    def arm_a():
        t0 = time.perf_counter()
        for i, (fk, ak, ck, mu) in enumerate(items):
            ctx.check(L.hb_verify_rhs(ctx.h, pb, len(pb), S, fk, ak, 32, chunks, ck, 32, chunks, pb, len(pb), mu,
                                      rhs1[i]))
        return time.perf_counter() - t0

    def arm_b():
        t0 = time.perf_counter()
        ctx.check(L.hb_verify_rhs_many(ctx.h, pb, len(pb), S, 32, 32, descs, nproofs, 0))
        return time.perf_counter() - t0

    arm_a()   # warm-up, and the results to compare
    arm_b()
    equal = ra.raw == rb.raw and len(set(ra.raw[i * w:(i + 1) * w] for i in range(nproofs))) == nproofs
    if not equal:
        raise SystemExit("the batch's right-hand sides differ from the loop's")
    a, b = [], []
    for _ in range(rounds):
        a.append(arm_a())
        b.append(arm_b())
    return report("%s-bit S=%d, %d proofs x %d chunks" % (bits, S, nproofs, chunks), a, b,
                  {"rhs_equal": equal, "A_us_per_proof": round(min(a) / nproofs * 1e6, 1),
                   "B_us_per_proof": round(min(b) / nproofs * 1e6, 1)})


def api_shape(rounds, bits=1024, S=10, nproofs=256, chunks=820):
    from heartbeat_amd.PySwizzle import PySwizzle
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["State"])
    p = prime(bits)
    w = nat.width_of(p)
    beat = PySwizzle(S, b"k" * 32, p)
    raw = proofs_of(p, S, nproofs, chunks)
    mus = [[int.from_bytes(mu[j * w:(j + 1) * w], "big") for j in range(S)] for _, _, _, mu in raw]
    # honest sigmas from the batch itself (checked against the loop below);
    # every fourth proof is left wrong
    sig = pys.verify_rhs_many(p, S, [(fk, ak, chunks, ck, chunks, p, m) for (fk, ak, ck, _), m in zip(raw, mus)])
    items = []
    for i, ((fk, ak, ck, _), m) in enumerate(zip(raw, mus)):
        proof = pys.Proof()
        proof.mu, proof.sigma = m, sig[i] if i % 4 else (sig[i] + 1) % p
        state = pys.State(fk, ak, chunks)
        state.encrypt(beat.key)
        items.append((proof, pys.Challenge(chunks, p, ck), state))

    def arm_a():
        t0 = time.perf_counter()
        res = [beat.verify(*it) for it in items]
        return time.perf_counter() - t0, res

    def arm_b():
        t0 = time.perf_counter()
        res = beat.verify_many(items)
        return time.perf_counter() - t0, res

    _, wa = arm_a()
    _, wb = arm_b()
    equal = wa == wb == [bool(i % 4) for i in range(nproofs)]
    if not equal:
        raise SystemExit("verify_many differs from the loop of verify")
    a, b = [], []
    for _ in range(rounds):
        a.append(arm_a()[0])
        b.append(arm_b()[0])
    return report("%d-bit S=%d, %d proofs x %d chunks (PySwizzle.verify_many vs verify loop)" % (bits, S, nproofs, chunks),
                  a, b, {"results_equal": equal})


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
            bits, S, n, chunks = s.split(":")
            rows.append(abi_shape(bits if bits == "P256" else int(bits), int(S), int(n), int(chunks), rounds))
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
