"""Re-tagging listed blocks with the cxx Swizzle against what there was before
(DESIGN.md 5.3l).  Per row, B's tags are compared with A's before any timing;
then one warm-up of both arms and alternating rounds of A and B, each timed
with a host clock around calls that end in a stream synchronise; min ... max.

At the cxx defaults (1024-bit prime, S = 10), a 1 GiB file in host memory:

  blocks:k    B: one hb_cxx_encode_blocks of k scattered blocks (k = 1, 64,
              4096), packed beforehand;
              A: a loop of hb_encode(HB_PRF_CXX, block_base = i, nblocks = 1)
              per listed block -- what the same keys offered before;
              A_whole: hb_encode(HB_PRF_CXX) of the whole file;
              B_patch: Swizzle.encode_blocks (the owner's side, Python and the
              packing included); B_update: Swizzle.update, which adds the copy
              of the server's tag that patch_tag makes and the new state.
  append      the same after 1 MiB was appended (the old last block and the
              new ones).
  many:n      B: one hb_cxx_encode_blocks_many of n files x 4 blocks, each file
              under its own keys; A: the loop of n x 4 hb_encode(HB_PRF_CXX).
              Host memory and device-resident.

  python scripts/cxx_blocks_rate.py [--rounds 5] [--gib 1] [--out FILE]
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
from heartbeat_amd import Swizzle as sw    # noqa: E402


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
    fn()
    return time.perf_counter() - t0


def rounds_of(arms, rounds):
    """One warm-up of every arm, then `rounds` alternating rounds."""
    for fn in arms.values():
        fn()
    ts = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ts[name].append(timed(fn))
    return ts


def file_rows(rounds, gib):
    p, S = prime(1024), 10
    beat = sw.Swizzle(1.0, S, True, p)
    w = nat.width_of(p)
    C = S * beat.sectorsize
    size, extra = int(gib * (1 << 30)), 1 << 20
    buf = np.random.default_rng(7).integers(0, 256, size + extra, dtype=np.uint8)
    fk, ak = hashlib.sha256(b"f").digest(), hashlib.sha256(b"a").digest()
    ctx = nat.context()
    ctx.prepare(p.bit_length())
    L = nat.lib()
    pb = nat.be(p)
    tries = ctypes.c_uint64()

    def whole(length, out):
        ctx.check(L.hb_encode(ctx.h, pb, len(pb), S, fk, ak, 32, 0, buf.ctypes.data, length, length // C + 1,
                              out.ctypes.data, nat.HB_PRF_CXX, None))

    n = size // C + 1
    tags = np.empty(n * w, dtype=np.uint8)
    whole(size, tags)
    tag = sw.Tag._from_raw(memoryview(tags), w)
    state = sw.State()
    state.n, state.f_key, state.alpha_key = n, fk, ak
    state.encrypt(beat.k_enc, beat.k_mac)
    rows = []
    rng = random.Random(3)
    cases = [("update of %d scattered blocks" % k, k, size) for k in (1, 64, 4096)]
    cases.append(("append of %d bytes" % extra, None, size + extra))
    for what, k, length in cases:
        n_new = length // C + 1
        if k is None:
            idx = list(range(n - 1, n_new))
        else:
            idx = sorted(rng.sample(range(n - 1), k))
            for i in idx:
                buf[i * C + 3] ^= 0x41
        lens = [min(C, length - i * C) for i in idx]
        blocks = [(i, buf[i * C:i * C + m].tobytes()) for i, m in zip(idx, lens)]
        packed = np.frombuffer(b"".join(d for _, d in blocks), dtype=np.uint8)
        ia = np.array(idx, dtype=np.uint64)
        out_a = np.zeros(len(idx) * w, dtype=np.uint8)
        out_b = np.zeros(len(idx) * w, dtype=np.uint8)
        out_w = np.empty(n_new * w, dtype=np.uint8)

        def arm_a():
            for j, (i, m) in enumerate(zip(idx, lens)):
                ctx.check(L.hb_encode(ctx.h, pb, len(pb), S, fk, ak, 32, i, buf.ctypes.data + i * C if m else None, m, 1,
                                      out_a.ctypes.data + j * w, nat.HB_PRF_CXX, ctypes.byref(tries)))

        def arm_b():
            ctx.check(L.hb_cxx_encode_blocks(ctx.h, pb, len(pb), S, fk, ak, 32, ia.ctypes.data, len(idx),
                                             packed.ctypes.data if len(packed) else None, len(packed), out_b.ctypes.data, 0,
                                             ctypes.byref(tries)))

        arm_a()
        arm_b()
        whole(length, out_w)
        rows_w = out_w.reshape(n_new, w)
        got = beat.update(tag, state, blocks, length)[0]
        equal = out_a.tobytes() == out_b.tobytes() and bool(out_a.any()) and \
            out_b.tobytes() == rows_w[idx].tobytes() and bytes(got.raw(p)) == out_w.tobytes()
        if not equal:
            raise SystemExit("%s: the tags differ" % what)
        arm_b()
        launches = ctx.last_kernel_ms()[1]
        ts = rounds_of({"A": arm_a, "B": arm_b, "A_whole": lambda: whole(length, out_w),
                        "B_patch": lambda: beat.encode_blocks(state, blocks),
                        "B_update": lambda: beat.update(tag, state, blocks, length)}, rounds)
        rows.append(report("1024-bit S=10, %d bytes host file, %s (%d blocks listed)" % (size, what, len(idx)), ts,
                           {"tags_equal": equal, "blocks": n_new, "launches_B": launches}))
        if k is not None:
            tags = out_w.copy()
            tag = sw.Tag._from_raw(memoryview(tags), w)
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
                        for k in range(per_file):
                            ctx.check(L.hb_encode(ctx.h, pb, len(pb), S, keys[i][0], keys[i][1], 32, int(idx[i][k]),
                                                  dbase + (i * per_file + k) * C, C, 1, tbase + (i * per_file + k) * w,
                                                  flags | nat.HB_PRF_CXX, ctypes.byref(tries)))

                def arm_b():
                    ctx.check(L.hb_cxx_encode_blocks_many(ctx.h, pb, len(pb), S, 32, descs, n, flags, ctypes.byref(tries)))

                arm_a()
                if device:
                    ctx.check(L.hb_memcpy(ctx.h, out_a.ctypes.data, t, len(out_a), 2))
                arm_b()
                if device:
                    ctx.check(L.hb_memcpy(ctx.h, out_b.ctypes.data, t, len(out_b), 2))
                equal = out_a.tobytes() == out_b.tobytes() and bool(out_a.any())
                if not equal:
                    raise SystemExit("the batch's tags differ from the loop's (%d files)" % n)
                launches = ctx.last_kernel_ms()[1]
                ts = rounds_of({"A": arm_a, "B": arm_b}, rounds)
                rows.append(report("1024-bit S=10, %d files x %d blocks (%s)" % (n, per_file, "device" if device else "host"),
                                   ts, {"tags_equal": equal, "launches_B": launches}))
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
    rows = many_rows(rounds, [1, 2, 4, 256]) + file_rows(rounds, gib)
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
