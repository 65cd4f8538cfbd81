"""The mixed-owner encodes against what a process with many beats can do without
them.  The shape is PySwizzle's defaults and the cxx Swizzle's
(1024-bit primes, S = 10), 256 files of 1 MiB, device-resident and from host
memory; per owner layout

  distinct: 256 distinct primes;   owners16: 16 owners x 16 files;   one: one prime

the arms

  A_loop    a loop of hb_encode (--cxx: with HB_PRF_CXX), one call per file (distinct, owners16);
  A_many    a loop of 16 hb_encode_many (--cxx: hb_cxx_encode_many), one per owner (owners16);
            one such call (one);
  B_mixed   one hb_encode_mixed (--cxx: hb_cxx_encode_mixed) (every layout);

each timed with a host clock around calls that return after the stream is
synchronised.  B's tags and tries are compared with the loop's before any
timing.

The A arms use only entry points from before the mixed calls, so they can run
on a build of the parent commit ($HB_LIB_PATH) while B runs on this tree's:

  python scripts/encode_mixed_rate.py [--cxx] [--rounds 7] [--out FILE]        A and B alternating, one process
  python scripts/encode_mixed_rate.py --arms A --rounds 1 --append A.jsonl   only the A arms (any build)
  python scripts/encode_mixed_rate.py --arms B --rounds 1 --append B.jsonl   only the B arm
  python scripts/encode_mixed_rate.py --merge A.jsonl B.jsonl --out FILE     rows from alternating runs of the two

  --primes FILE   cache of the generated primes (hex, JSON): made on the first run
  --files N       files per call (default 256; owners16 needs a multiple of 16; 1, 2, 3: the threshold rows,
                  which run the distinct layout only)
"""
import ctypes
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402

MIB = 1 << 20
BITS, S, LENGTH = 1024, 10, MIB
LAYOUTS = ("distinct", "owners16", "one")


def make_primes(n, path):
    if path and os.path.exists(path):
        with open(path) as fh:
            have = [int(x, 16) for x in json.load(fh)]
        if len(have) >= n:
            return have[:n]
    pys = __import__("heartbeat_amd.PySwizzle.PySwizzle", fromlist=["_is_probable_prime"])
    rng = random.Random(7000 + BITS)
    out = []
    while len(out) < n:
        x = rng.getrandbits(BITS) | (1 << (BITS - 1)) | 1
        if pys._is_probable_prime(x) and x not in out:
            out.append(x)
    if path:
        with open(path, "w") as fh:
            json.dump(["%x" % x for x in out], fh)
    return out


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
            "spread_ms": round((max(ts) - min(ts)) * 1e3, 3), "rounds": len(ts)}


def key_of(tag, i):
    return hashlib.sha256(b"%s/%d" % (tag, i)).digest()


class Dev(object):
    """One device allocation, filled with seeded bytes (hb_fill_random) when a seed is given."""

    def __init__(self, ctx, n, seed=None):
        self.ctx, self.n = ctx, n
        p = ctypes.c_void_p()
        ctx.check(nat.lib().hb_device_malloc(ctx.h, n, ctypes.byref(p)))
        self.p = p.value
        if seed is not None:
            ctx.check(nat.lib().hb_fill_random(ctx.h, self.p, n, seed))

    def download(self):
        out = np.empty(self.n, dtype=np.uint8)
        self.ctx.check(nat.lib().hb_memcpy(self.ctx.h, out.ctypes.data, self.p, self.n, 2))
        return out

    def free(self):
        self.ctx.check(nat.lib().hb_device_free(self.ctx.h, self.p))


def owners_of(layout, n, primes):
    """The prime of every file."""
    if layout == "distinct":
        return [primes[i] for i in range(n)]
    if layout == "owners16":
        return [primes[i // (n // 16)] for i in range(n)]
    return [primes[0]] * n


def encode_arms(ctx, L, layout, n, primes, where, arms, cxx):
    """{arm: callable -> seconds}, and a check of B against the loop."""
    ps = owners_of(layout, n, primes)
    pbs = [nat.be(p) for p in ps]
    w = nat.width_of(ps[0])
    C = (BITS // 8) * S
    nb = LENGTH // C + 1
    dstride, tstride = (LENGTH + 15) & ~15, (nb * w + 15) & ~15
    ddev = Dev(ctx, dstride * n + 16, 0x5EED0100)
    flags = 0 if where == "host" else 3
    single_flags = flags | (nat.HB_PRF_CXX if cxx else 0)
    hold, devs = [], [ddev]
    if flags:
        ta, tb = Dev(ctx, tstride * n + 16), Dev(ctx, tstride * n + 16)
        devs += [ta, tb]
        dbase, a0, b0 = ddev.p, ta.p, tb.p
        tags_of = lambda d: d.download().tobytes()   # noqa: E731
        ra, rb = ta, tb
    else:
        dhost = ddev.download()
        ra, rb = np.zeros(tstride * n, dtype=np.uint8), np.zeros(tstride * n, dtype=np.uint8)
        hold += [dhost, ra, rb]
        dbase, a0, b0 = dhost.ctypes.data, ra.ctypes.data, rb.ctypes.data
        tags_of = lambda a: a.tobytes()   # noqa: E731
    fks, aks = [key_of(b"f", i) for i in range(n)], [key_of(b"a", i) for i in range(n)]
    tries = ctypes.c_uint64()
    seen = {}

    def fill(d, i, base):
        d.f_key, d.alpha_key = fks[i], aks[i]
        d.data, d.len = dbase + i * dstride, LENGTH
        d.tags = base + i * tstride

    def loop():
        total = 0
        t0 = time.perf_counter()
        for i in range(n):
            ctx.check(L.hb_encode(ctx.h, pbs[i], len(pbs[i]), S, fks[i], aks[i], 32, 0, dbase + i * dstride, LENGTH, nb,
                                  a0 + i * tstride, single_flags, ctypes.byref(tries)))
            total += tries.value
        dt = time.perf_counter() - t0
        seen["A"] = total
        return dt

    out = {}
    many_fn = getattr(L, "hb_cxx_encode_many" if cxx else "hb_encode_many")
    if "A" in arms:
        if layout != "one":
            out["A_loop"] = loop
        if layout != "distinct":
            per = n // 16 if layout == "owners16" else n
            descs = (nat.FileDesc * n)()
            for i in range(n):
                fill(descs[i], i, a0)
            hold.append(descs)

            def many():
                t0 = time.perf_counter()
                for o in range(0, n, per):
                    sub = ctypes.cast(ctypes.byref(descs, o * ctypes.sizeof(nat.FileDesc)), ctypes.POINTER(nat.FileDesc))
                    ctx.check(many_fn(ctx.h, pbs[o], len(pbs[o]), S, 32, sub, per, flags, ctypes.byref(tries)))
                return time.perf_counter() - t0
            out["A_many"] = many
    check = None
    if "B" in arms:
        mixed_fn = getattr(L, "hb_cxx_encode_mixed" if cxx else "hb_encode_mixed")
        md = (nat.EncodeMixedDesc * n)()
        for i in range(n):
            md[i].p_be, md[i].p_len, md[i].sectors, md[i].key_len = pbs[i], len(pbs[i]), S, 32
            fill(md[i], i, b0)
        hold.append(md)

        def mixed():
            t0 = time.perf_counter()
            ctx.check(mixed_fn(ctx.h, md, n, flags, ctypes.byref(tries)))
            dt = time.perf_counter() - t0
            seen["B"] = tries.value
            return dt
        out["B_mixed"] = mixed

        def check():
            loop()
            mixed()
            a, b = tags_of(ra), tags_of(rb)
            used = [a[i * tstride:i * tstride + nb * w] for i in range(n)]
            return (used == [b[i * tstride:i * tstride + nb * w] for i in range(n)] and len(set(used)) == n and
                    seen["A"] == seen["B"] and seen["A"] >= n * nb)
    return out, check, lambda: [d.free() for d in devs], hold


def run(arms, rounds, n, primes_path, append, cxx):
    ctx = nat.context()
    L = nat.lib()
    ctx.prepare(BITS)
    primes = make_primes(n, primes_path)
    rows = []
    layouts = LAYOUTS if n % 16 == 0 else ("distinct",)
    for where in ("dev", "host"):
        for layout in layouts:
            fns, check, free, hold = encode_arms(ctx, L, layout, n, primes, where, arms, cxx)
            try:
                equal = None
                if check:
                    equal = check()
                    if not equal:
                        raise SystemExit("%s %s: the mixed call's tags or tries differ from the loop's" % (where, layout))
                for fn in fns.values():   # warm-up of every arm
                    fn()
                times = {k: [] for k in fns}
                for _ in range(rounds):   # alternating
                    for k, fn in fns.items():
                        times[k].append(fn())
            finally:
                free()
            row = {"what": "cxx_encode" if cxx else "encode", "where": where, "layout": layout, "bits": BITS, "S": S,
                   "files": n, "length": LENGTH, "arms": arms, "times_s": times, "results_equal": equal,
                   "build_id": nat.build_info()["build_id"]}
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "times_s"}, sort_keys=True),
                  {k: round(min(v) * 1e3, 3) for k, v in times.items()}, flush=True)
    if append:
        with open(append, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    return rows


def summarise(rows):
    """One row per (what, where, layout, files) from any number of runs' rows."""
    acc = {}
    for r in rows:
        k = (r["what"], r["where"], r["layout"], r["files"])
        e = acc.setdefault(k, {"what": r["what"], "where": r["where"], "layout": r["layout"], "bits": r["bits"], "S": r["S"],
                               "files": r["files"], "length": r["length"], "times": {}, "builds": {}})
        for arm, ts in r["times_s"].items():
            e["times"].setdefault(arm, []).extend(ts)
            e["builds"][arm] = r["build_id"]
        if r.get("results_equal") is not None:
            e["results_equal"] = r["results_equal"]
    out = []
    for e in acc.values():
        t = e.pop("times")
        for arm, ts in t.items():
            e[arm] = stats(ts)
        if "B_mixed" in t:
            b = t["B_mixed"]
            for arm in ("A_loop", "A_many"):
                if arm in t:
                    e["B_slowest_beats_%s_fastest" % arm] = max(b) < min(t[arm])
                    e["ratio_min_%s_over_min_B" % arm] = round(min(t[arm]) / min(b), 2)
            if e["layout"] == "one" and "A_many" in t:   # what reading the modulus from a table costs: a figure, not a gate
                margin = max(max(b) - min(b), max(t["A_many"]) - min(t["A_many"]))
                e["one_prime_margin_ms"] = round(margin * 1e3, 3)
                e["one_prime_B_minus_A_ms"] = round((min(b) - min(t["A_many"])) * 1e3, 3)
                e["one_prime_within_margin"] = abs(min(b) - min(t["A_many"])) <= margin
        out.append(e)
    for e in out:
        print(json.dumps(e, sort_keys=True), flush=True)
    return out


def main(argv):
    rounds, out, arms, n, primes_path, append, merge, cxx = 7, None, "AB", 256, None, None, [], False
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        elif x == "--arms":
            arms = next(it)
        elif x == "--files":
            n = int(next(it))
        elif x == "--primes":
            primes_path = next(it)
        elif x == "--append":
            append = next(it)
        elif x == "--merge":
            merge = [next(it), next(it)]
        elif x == "--cxx":
            cxx = True
        else:
            raise SystemExit("unknown argument %s" % x)
    if merge:
        rows = []
        for path in merge:
            with open(path) as fh:
                rows += [json.loads(ln) for ln in fh if ln.strip()]
    else:
        rows = run(arms, rounds, n, primes_path, append, cxx)
    if out or merge or arms == "AB":
        res = summarise(rows)
        if out:
            with open(out, "w") as fh:
                json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
