"""The cxx mixed-owner batches against what a node with many owners of the cxx
Swizzle can do without them.  Per shape -- the cxx defaults:
1024-bit, S = 10, 256 proofs over 1 MiB files of 820 blocks, at check_fraction
1.0 (820 chunks: check_all) and 0.3 (246 sampled chunks), prove with the data
device-resident and from host memory, and verify -- and per owner layout

  distinct: 256 distinct primes;   owners16: 16 owners x 16 proofs;   one: one prime

the arms

  A_loop    a loop of hb_prove(HB_PRF_CXX) / hb_cxx_verify_rhs, one call per proof (distinct, owners16);
  A_many    a loop of 16 hb_cxx_prove_many / hb_cxx_verify_rhs_many, one per owner (owners16);
            one hb_cxx_prove_many / hb_cxx_verify_rhs_many (one);
  B_mixed   one hb_cxx_prove_mixed / hb_cxx_verify_rhs_mixed (every layout);

each timed with a host clock around calls that return after the stream is
synchronised.  B's results are compared with the loop's before any timing.

The A arms use only entry points from before the cxx mixed calls, so they can
run on a build of the parent commit ($HB_LIB_PATH) while B runs on this tree's:

  python scripts/cxx_mixed_many_rate.py [--rounds 7] [--out FILE]           A and B alternating, one process
  python scripts/cxx_mixed_many_rate.py --arms A --rounds 1 --append A.jsonl   only the A arms (any build)
  python scripts/cxx_mixed_many_rate.py --arms B --rounds 1 --append B.jsonl   only the B arm
  python scripts/cxx_mixed_many_rate.py --merge A.jsonl B.jsonl --out FILE   rows from alternating runs of the two

  --primes FILE   cache of the generated primes (hex, JSON): made on the first run
  --proofs N      proofs per call (default 256; owners16 needs a multiple of 16 and is
                  left out otherwise: the 1-, 2- and 3-proof rows behind the Python
                  thresholds CXX_PROVE_MANY_MIN / CXX_VERIFY_MANY_MIN)
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
NTAGS = LENGTH // ((BITS // 8) * S) + 1          # 820 blocks
FRACTIONS = (1.0, 0.3)
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


def owners_of(layout, n, primes):
    """The prime of every proof, and the runs of proofs of one owner."""
    if layout == "distinct":
        return [primes[i] for i in range(n)]
    if layout == "owners16":
        return [primes[i // (n // 16)] for i in range(n)]
    return [primes[0]] * n


def prove_arms(ctx, L, layout, n, primes, where, arms, CHUNKS):
    """{arm: callable -> seconds}, and a check of B against the loop."""
    ps = owners_of(layout, n, primes)
    pbs = [nat.be(p) for p in ps]
    w = nat.width_of(ps[0])
    C = (BITS // 8) * S
    ntags = LENGTH // C + 1
    dstride, tstride = (LENGTH + 15) & ~15, (ntags * w + 15) & ~15
    ddev, tdev = Dev(ctx, dstride * n + 16, 0x5EED0100), Dev(ctx, tstride * n + 16, 0x5EED0200)
    flags = 0 if where == "host" else 3
    hold = [ddev, tdev]
    if flags:
        dbase, tbase = ddev.p, tdev.p
    else:
        dhost, thost = ddev.download(), tdev.download()
        hold += [dhost, thost]
        dbase, tbase = dhost.ctypes.data, thost.ctypes.data
    n1 = (S + 1) * w
    ra, rb = ctypes.create_string_buffer(n * n1), ctypes.create_string_buffer(n * n1)
    keys = [key_of(b"c", i) for i in range(n)]
    a0, b0 = ctypes.addressof(ra), ctypes.addressof(rb)
    hold += [ra, rb]   # the arms hold addresses only

    def fill(d, i, base):
        d.chal_key, d.chunks = keys[i], CHUNKS
        d.vmax_be, d.vmax_len = pbs[i], len(pbs[i])
        d.tags, d.ntags = tbase + i * tstride, ntags
        d.data, d.len = dbase + i * dstride, LENGTH
        d.mu_out, d.sigma_out = base + i * n1, base + i * n1 + S * w

    def loop():
        t0 = time.perf_counter()
        for i in range(n):
            ctx.check(L.hb_prove(ctx.h, pbs[i], len(pbs[i]), S, keys[i], 32, CHUNKS, pbs[i], len(pbs[i]), tbase + i * tstride,
                                 ntags, dbase + i * dstride, LENGTH, flags | nat.HB_PRF_CXX, a0 + i * n1, a0 + i * n1 + S * w))
        return time.perf_counter() - t0

    out = {}
    if "A" in arms:
        if layout != "one":
            out["A_loop"] = loop
        if layout != "distinct":
            per = n // 16 if layout == "owners16" else n
            descs = (nat.ProveDesc * n)()
            for i in range(n):
                fill(descs[i], i, a0)
            hold.append(descs)

            def many():
                t0 = time.perf_counter()
                for o in range(0, n, per):
                    sub = ctypes.cast(ctypes.byref(descs, o * ctypes.sizeof(nat.ProveDesc)), ctypes.POINTER(nat.ProveDesc))
                    ctx.check(L.hb_cxx_prove_many(ctx.h, pbs[o], len(pbs[o]), S, 32, sub, per, flags))
                return time.perf_counter() - t0
            out["A_many"] = many
    check = None
    if "B" in arms:
        md = (nat.ProveMixedDesc * n)()
        for i in range(n):
            md[i].p_be, md[i].p_len, md[i].sectors, md[i].key_len = pbs[i], len(pbs[i]), S, 32
            fill(md[i], i, b0)
        hold.append(md)

        def mixed():
            t0 = time.perf_counter()
            ctx.check(L.hb_cxx_prove_mixed(ctx.h, md, n, flags))
            return time.perf_counter() - t0
        out["B_mixed"] = mixed

        def check():
            loop()
            mixed()
            return ra.raw == rb.raw and len(set(ra.raw[i * n1:(i + 1) * n1] for i in range(n))) == n
    return out, check, lambda: (ddev.free(), tdev.free()), hold


def verify_arms(ctx, L, layout, n, primes, arms, CHUNKS):
    ps = owners_of(layout, n, primes)
    pbs = [nat.be(p) for p in ps]
    w = nat.width_of(ps[0])
    rng = np.random.default_rng(0x5EED)
    fks, aks, cks = ([key_of(t, i) for i in range(n)] for t in (b"f", b"a", b"c"))
    mus = [b"".join((int.from_bytes(rng.integers(0, 256, w, dtype=np.uint8).tobytes(), "big") % ps[i]).to_bytes(w, "big")
                    for _ in range(S)) for i in range(n)]
    ra, rb = ctypes.create_string_buffer(n * w), ctypes.create_string_buffer(n * w)
    a0, b0 = ctypes.addressof(ra), ctypes.addressof(rb)
    hold = [mus, ra, rb]   # the arms hold addresses only

    def fill(d, i, base):
        d.f_key, d.alpha_key, d.chal_key = fks[i], aks[i], cks[i]
        d.state_chunks, d.chunks = NTAGS, CHUNKS
        d.vmax_be, d.vmax_len = pbs[i], len(pbs[i])
        d.mu = mus[i]
        d.rhs_out = base + i * w

    def loop():
        t0 = time.perf_counter()
        for i in range(n):
            ctx.check(L.hb_cxx_verify_rhs(ctx.h, pbs[i], len(pbs[i]), S, fks[i], aks[i], 32, NTAGS, cks[i], 32, CHUNKS, pbs[i],
                                      len(pbs[i]), mus[i], a0 + i * w))
        return time.perf_counter() - t0

    out = {}
    if "A" in arms:
        if layout != "one":
            out["A_loop"] = loop
        if layout != "distinct":
            per = n // 16 if layout == "owners16" else n
            descs = (nat.VerifyDesc * n)()
            for i in range(n):
                fill(descs[i], i, a0)
            hold.append(descs)

            def many():
                t0 = time.perf_counter()
                for o in range(0, n, per):
                    sub = ctypes.cast(ctypes.byref(descs, o * ctypes.sizeof(nat.VerifyDesc)), ctypes.POINTER(nat.VerifyDesc))
                    ctx.check(L.hb_cxx_verify_rhs_many(ctx.h, pbs[o], len(pbs[o]), S, 32, 32, sub, per, 0))
                return time.perf_counter() - t0
            out["A_many"] = many
    check = None
    if "B" in arms:
        md = (nat.VerifyMixedDesc * n)()
        for i in range(n):
            md[i].p_be, md[i].p_len, md[i].sectors, md[i].key_len, md[i].chal_key_len = pbs[i], len(pbs[i]), S, 32, 32
            fill(md[i], i, b0)
        hold.append(md)

        def mixed():
            t0 = time.perf_counter()
            ctx.check(L.hb_cxx_verify_rhs_mixed(ctx.h, md, n, 0))
            return time.perf_counter() - t0
        out["B_mixed"] = mixed

        def check():
            loop()
            mixed()
            return ra.raw == rb.raw and len(set(ra.raw[i * w:(i + 1) * w] for i in range(n))) == n
    return out, check, lambda: None, hold


def run(arms, rounds, n, primes_path, append):
    ctx = nat.context()
    L = nat.lib()
    ctx.prepare(BITS)
    primes = make_primes(n, primes_path)
    rows = []
    layouts = [x for x in LAYOUTS if x != "owners16" or n % 16 == 0]
    for what, where, fraction in [(a, b, f) for a, b in (("prove", "dev"), ("prove", "host"), ("verify", "host")) for f in FRACTIONS]:
        chunks = int(fraction * NTAGS)
        for layout in layouts:
            if what == "prove":
                fns, check, free, hold = prove_arms(ctx, L, layout, n, primes, where, arms, chunks)
            else:
                fns, check, free, hold = verify_arms(ctx, L, layout, n, primes, arms, chunks)
            try:
                equal = None
                if check:
                    equal = check()
                    if not equal:
                        raise SystemExit("%s %s %s %s: the mixed call's results differ from the loop's" % (what, where, layout, fraction))
                for fn in fns.values():   # warm-up of every arm
                    fn()
                times = {k: [] for k in fns}
                for _ in range(rounds):   # alternating
                    for k, fn in fns.items():
                        times[k].append(fn())
            finally:
                free()
            row = {"what": what, "where": where if what == "prove" else "host", "layout": layout, "bits": BITS, "S": S,
                   "proofs": n, "chunks": chunks, "check_fraction": fraction, "arms": arms, "times_s": times,
                   "results_equal": equal, "build_id": nat.build_info()["build_id"]}
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "times_s"}, sort_keys=True),
                  {k: round(min(v) * 1e3, 3) for k, v in times.items()}, flush=True)
    if append:
        with open(append, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    return rows


def summarise(rows):
    """One row per (what, where, layout) from any number of runs' rows."""
    acc = {}
    for r in rows:
        k = (r["what"], r["where"], r["check_fraction"], r["proofs"], r["layout"])
        e = acc.setdefault(k, {"what": r["what"], "where": r["where"], "layout": r["layout"], "bits": r["bits"], "S": r["S"],
                               "proofs": r["proofs"], "chunks": r["chunks"], "check_fraction": r["check_fraction"],
                               "times": {}, "builds": {}})
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
            if e["layout"] == "one" and "A_many" in t:
                margin = max(max(b) - min(b), max(t["A_many"]) - min(t["A_many"]))
                e["one_prime_margin_ms"] = round(margin * 1e3, 3)
                e["one_prime_B_minus_A_ms"] = round((min(b) - min(t["A_many"])) * 1e3, 3)
                e["one_prime_within_margin"] = abs(min(b) - min(t["A_many"])) <= margin
        out.append(e)
    by = {(e["what"], e["where"], e["check_fraction"], e["proofs"], e["layout"]): e for e in out}
    for (what, where, fraction, n, layout), e in by.items():   # what a distinct prime costs on the host: distinct against one
        one = by.get((what, where, fraction, n, "one"))
        if layout == "distinct" and one and "B_mixed" in e and "B_mixed" in one:
            e["B_distinct_minus_one_ms"] = round(e["B_mixed"]["min_ms"] - one["B_mixed"]["min_ms"], 3)
            if e["proofs"] > 1:
                e["B_us_per_distinct_prime"] = round(1e3 * e["B_distinct_minus_one_ms"] / (e["proofs"] - 1), 2)
    for e in out:
        print(json.dumps(e, sort_keys=True), flush=True)
    return out


def main(argv):
    rounds, out, arms, n, primes_path, append, merge = 7, None, "AB", 256, None, None, []
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        elif x == "--arms":
            arms = next(it)
        elif x == "--proofs":
            n = int(next(it))
        elif x == "--primes":
            primes_path = next(it)
        elif x == "--append":
            append = next(it)
        elif x == "--merge":
            merge = [next(it), next(it)]
        else:
            raise SystemExit("unknown argument %s" % x)
    if merge:
        rows = []
        for path in merge:
            with open(path) as fh:
                rows += [json.loads(ln) for ln in fh if ln.strip()]
    else:
        rows = run(arms, rounds, n, primes_path, append)
    if out or merge or arms == "AB":
        res = summarise(rows)
        if out:
            with open(out, "w") as fh:
                json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
