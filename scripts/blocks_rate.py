"""Re-tagging listed blocks against a full encode.  Per row,
after a warm-up of both arms, alternating rounds of A and B, each timed with a
host clock around calls that end in a stream synchronise; min ... max of both.

At PySwizzle's defaults (1024-bit prime, S = 10), a 1 GiB file in host memory:

  update:k    B: PySwizzle.update of k scattered blocks (k = 1, 64, 4096), and
              B_patch: encode_blocks alone -- the owner's side, without the
              copy of the server's tag that patch_tag makes;
              A: encode_file of the whole new file under the same keys, which
              is what a changed block costs without this call.
  append      B: update after 1 MiB was appended; A: encode_file of the new file.
  many:n      B: one hb_encode_blocks_many of n files x 4 blocks, each file
              under its own keys; A: a loop of n hb_encode_blocks.  Host
              memory and device-resident.  PySwizzle.update_many against a loop
              of update differ by exactly these calls.

B's tags are compared with A's before any timing.

  python scripts/blocks_rate.py [--rounds 5] [--gib 1] [--out FILE]
"""
import ctypes
import hashlib
import json
import random
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402


def prime(bits):
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["_is_probable_prime"])
    rng = random.Random(5000 + bits)
    while True:
        x = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if pys._is_probable_prime(x):
            return x


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def report(shape, arms, extra):
    row = {"shape": shape}
    for name, ts in arms.items():
        row[name] = stats(ts)
    a, b = arms["A"], arms["B"]
    row["ratio_minA_over_maxB"] = round(min(a) / max(b), 2)
    row["ratio_min_over_min"] = round(min(a) / min(b), 2)
    row["B_slowest_beats_A_fastest"] = max(b) < min(a)
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def file_rows(rounds, gib):
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["PySwizzle"])
    p, S = prime(1024), 10
    beat = pys.PySwizzle(S, b"k" * 32, p)
    C = S * beat.sectorsize
    size, extra = int(gib * (1 << 30)), 1 << 20
    buf = np.random.default_rng(7).integers(0, 256, size + extra, dtype=np.uint8)
    old = memoryview(buf)[:size]
    fk, ak = hashlib.sha256(b"f").digest(), hashlib.sha256(b"a").digest()
    ctx = nat.context()
    ctx.prepare(p.bit_length())
    tag, n = pys.encode_file(p, S, fk, ak, old)
    state = pys.State(fk, ak, n)
    state.encrypt(beat.key)
    rows = []
    rng = random.Random(3)
    for k in (1, 64, 4096):
        idx = rng.sample(range(n - 1), k)
        for i in idx:
            buf[i * C + 3] ^= 0x41
        blocks = [(i, bytes(old[i * C:(i + 1) * C])) for i in idx]
        arm_a = lambda: pys.encode_file(p, S, fk, ak, old)[0]                    # noqa: E731
        arm_b = lambda: beat.update(tag, state, blocks)[0]                      # noqa: E731
        arm_p = lambda: beat.encode_blocks(state, blocks)                       # noqa: E731
        want = arm_a()
        got = arm_b()
        pidx, patch = arm_p()
        equal = bytes(got.raw(p)) == bytes(want.raw(p)) and \
            bytes(pys.PySwizzle.patch_tag(tag, pidx, patch).raw(p)) == bytes(want.raw(p))
        if not equal:
            raise SystemExit("update of %d blocks differs from the full encode" % k)
        a, b, pt = [], [], []
        for _ in range(rounds):
            a.append(timed(arm_a)[0])
            b.append(timed(arm_b)[0])
            pt.append(timed(arm_p)[0])
        rows.append(report("1024-bit S=10, %d bytes host file, update of %d scattered blocks" % (size, k),
                           {"A": a, "B": b, "B_patch": pt},
                           {"tags_equal": equal, "blocks": n, "phases_ms": ctx.last_kernel_phases(),
                            "launches": ctx.last_kernel_ms()[1]}))
        tag = want
    # append 1 MiB
    new = memoryview(buf)
    n_new = len(new) // C + 1
    blocks = [(i, bytes(new[i * C:(i + 1) * C])) for i in range(n - 1, n_new)]
    arm_a = lambda: pys.encode_file(p, S, fk, ak, new)[0]                        # noqa: E731
    arm_b = lambda: beat.update(tag, state, blocks, len(new))[0]                # noqa: E731
    arm_p = lambda: beat.encode_blocks(state, blocks)                           # noqa: E731
    want, got = arm_a(), arm_b()
    equal = bytes(got.raw(p)) == bytes(want.raw(p))
    if not equal:
        raise SystemExit("update after the append differs from the full encode")
    a, b, pt = [], [], []
    for _ in range(rounds):
        a.append(timed(arm_a)[0])
        b.append(timed(arm_b)[0])
        pt.append(timed(arm_p)[0])
    rows.append(report("1024-bit S=10, %d bytes host file, append of %d bytes (%d blocks)" % (size, extra, len(blocks)),
                       {"A": a, "B": b, "B_patch": pt},
                       {"tags_equal": equal, "phases_ms": ctx.last_kernel_phases(), "launches": ctx.last_kernel_ms()[1]}))
    return rows


def many_rows(rounds, counts, per_file=4):
    p, S = prime(1024), 10
    w = nat.width_of(p)
    C = (p.bit_length() // 8) * S
    ctx = nat.context()
    L = nat.lib()
    pb = nat.be(p)
    rows = []
    nmax = max(counts)
    keys = [(hashlib.sha256(b"f%d" % i).digest(), hashlib.sha256(b"a%d" % i).digest()) for i in range(nmax)]
    rng = random.Random(9)
    idx = [np.array(rng.sample(range(1 << 20), per_file), dtype=np.uint64) for _ in range(nmax)]
    host = np.random.default_rng(9).integers(0, 256, nmax * per_file * C, dtype=np.uint8)
    d, t = ctypes.c_void_p(), ctypes.c_void_p()
    ctx.check(L.hb_device_malloc(ctx.h, len(host), ctypes.byref(d)))
    ctx.check(L.hb_device_malloc(ctx.h, nmax * per_file * w, ctypes.byref(t)))
    ctx.check(L.hb_memcpy(ctx.h, d, host.ctypes.data, len(host), 1))
    try:
        for device in (False, True):
            for n in counts:
                out_a = np.zeros(n * per_file * w, dtype=np.uint8)
                out_b = np.zeros(n * per_file * w, dtype=np.uint8)
                flags = 3 if device else 0
                dbase = d.value if device else host.ctypes.data
                descs = (nat.BlocksDesc * n)()
                for i in range(n):
                    descs[i].f_key, descs[i].alpha_key = keys[i]
                    descs[i].indices, descs[i].nblocks = idx[i].ctypes.data, per_file
                    descs[i].data, descs[i].len = dbase + i * per_file * C, per_file * C
                    descs[i].tags = (t.value if device else out_b.ctypes.data) + i * per_file * w
                tries = ctypes.c_uint64()

                def arm_a():
                    tbase = t.value if device else out_a.ctypes.data
                    for i in range(n):
                        ctx.check(L.hb_encode_blocks(ctx.h, pb, len(pb), S, keys[i][0], keys[i][1], 32, idx[i].ctypes.data,
                                                     per_file, dbase + i * per_file * C, per_file * C,
                                                     tbase + i * per_file * w, flags, ctypes.byref(tries)))

                def arm_b():
                    ctx.check(L.hb_encode_blocks_many(ctx.h, pb, len(pb), S, 32, descs, n, flags, ctypes.byref(tries)))

                arm_a()
                if device:
                    ctx.check(L.hb_memcpy(ctx.h, out_a.ctypes.data, t, len(out_a), 2))
                arm_b()
                if device:
                    ctx.check(L.hb_memcpy(ctx.h, out_b.ctypes.data, t, len(out_b), 2))
                equal = out_a.tobytes() == out_b.tobytes() and bool(out_a.any())
                if not equal:
                    raise SystemExit("the batch's tags differ from the loop's (%d files)" % n)
                a, b = [], []
                for _ in range(rounds):
                    a.append(timed(arm_a)[0])
                    b.append(timed(arm_b)[0])
                rows.append(report("1024-bit S=10, %d files x %d blocks (%s)" % (n, per_file, "device" if device else "host"),
                                   {"A": a, "B": b}, {"tags_equal": equal, "launches_B": ctx.last_kernel_ms()[1]}))
    finally:
        ctx.check(L.hb_device_free(ctx.h, d))
        ctx.check(L.hb_device_free(ctx.h, t))
    return rows


def main(argv):
    rounds, out, gib = 5, None, 1.0
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        elif x == "--gib":
            gib = float(next(it))
    rows = many_rows(rounds, [1, 2, 3, 4, 256]) + file_rows(rounds, gib)
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
