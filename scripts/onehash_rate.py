"""OneHash: the batched GPU calls against loops of the host path.

The baseline of every shape is a loop of the class's forced host path
(HB_ONEHASH_HOST=1): the reference's own statements -- a seek, a read and a
hashlib.sha256 per challenge -- over files on disk.  The batch is the same
public call with the GPU path forced (HB_ONEHASH_DEVICE=1), from files on disk
("host": mapped, then uploaded or gathered) and device-resident
(OneHash.from_device).  After a warm-up of every arm and a check that all
arms give the same responses, `rounds` alternating rounds, each timed with a
host clock around calls that return synchronised; min ... max are reported,
and whether the batch's slowest round beats the loop's fastest.

  gen_one    generate_challenges(10000) on one 1 MiB file
  gen_many   generate_challenges_many for 256 files x 1000
  meet_files meet_many for 256 files x 1 challenge
  meet_one   meet_many for 1 file x 10000 challenges

Then the crossovers: "crossover_jobs" times meet_challenges and
generate_challenges of one 1 MiB file on disk at 1 ... 4096 jobs on both
forced paths (OH_DEVICE_MIN_JOBS, hb_onehash_host.hpp); "chain" times
generate_challenges_many of 1 ... 256 small device-resident files x 1000 with
the chains forced onto the host and onto the GPU (OH_CHAIN_DEVICE_MIN_FILES).

  python scripts/onehash_rate.py [--rounds 5] [--files 256] [--out FILE]
"""
import ctypes
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402
from heartbeat_amd.OneHash import Challenge, OneHash   # noqa: E402

MIB = 1 << 20
SECRET = b"mysecret"


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
            "spread_ms": round((max(ts) - min(ts)) * 1e3, 3)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def forced(path, f):
    """f() with the OneHash path forced: "host" or "device"."""
    def run():
        os.environ.pop("HB_ONEHASH_HOST", None)
        os.environ.pop("HB_ONEHASH_DEVICE", None)
        os.environ["HB_ONEHASH_" + path.upper()] = "1"
        try:
            return f()
        finally:
            os.environ.pop("HB_ONEHASH_" + path.upper(), None)
    return run


def compare(rounds, arms):
    """arms: name -> callable returning the responses ("loop" the baseline).
    Warm-up, equality, then alternating rounds."""
    first = {k: f() for k, f in arms.items()}
    for k, v in first.items():
        if v != first["loop"]:
            raise SystemExit("arm %s differs from the loop" % k)
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ts[k].append(clock(f)[0])
    row = {k: stats(v) for k, v in ts.items()}
    for k in arms:
        if k != "loop":
            row["%s_slowest_beats_loop_fastest" % k] = max(ts[k]) < min(ts["loop"])
            row["ratio_min_loop_over_max_%s" % k] = round(min(ts["loop"]) / max(ts[k]), 2)
    return row


def main(argv):
    rounds, out, nfiles = 5, None, 256
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        elif x == "--files":
            nfiles = int(next(it))
    ctx = nat.context()
    L = nat.lib()
    p = ctypes.c_void_p()
    ctx.check(L.hb_device_malloc(ctx.h, nfiles * MIB, ctypes.byref(p)))
    dev = p.value
    rows, on_disk = [], []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    with tempfile.TemporaryDirectory() as tmp:
        try:
            ctx.check(L.hb_fill_random(ctx.h, dev, nfiles * MIB, 0x5EED0500))
            host = np.empty(nfiles * MIB, dtype=np.uint8)
            ctx.check(L.hb_memcpy(ctx.h, host.ctypes.data, dev, nfiles * MIB, 2))
            paths = []
            for i in range(nfiles):
                paths.append(os.path.join(tmp, "f%d.bin" % i))
                host[i * MIB:(i + 1) * MIB].tofile(paths[-1])
            on_disk = [OneHash(q, SECRET) for q in paths]
            on_dev = [OneHash.from_device(dev + i * MIB, MIB, SECRET) for i in range(nfiles)]
            roots = [hashlib.sha256(b"onehash-rate-root/%d" % i).digest() for i in range(nfiles)]

            def responses(beats):
                return [c.response for b in beats for c in b.challenges]

            def gen_loop(beats, num):
                for b, r in zip(beats, roots):
                    b.generate_challenges(num, r)
                return responses(beats)

            def gen_many(beats, num):
                OneHash.generate_challenges_many([(b, num, r) for b, r in zip(beats, roots)])
                return responses(beats)

            build = nat.build_info()["build_id"]
            for what, k, num in (("gen_one", 1, 10000), ("gen_many", nfiles, 1000)):
                arms = {"loop": forced("host", lambda: gen_loop(on_disk[:k], num)),
                        "batch_host": forced("device", lambda: gen_many(on_disk[:k], num)),
                        "batch_dev": forced("device", lambda: gen_many(on_dev[:k], num))}
                row = {"what": what, "files": k, "file_bytes": MIB, "num": num, "rounds": rounds, "build": build}
                row.update(compare(rounds, arms))
                emit(row)

            gen_loop(on_disk, 1)
            one = [(b, b.challenges[0].without_answer) for b in on_disk]
            gen_loop(on_disk[:1], 10000)
            many = [(on_disk[0], c.without_answer) for c in on_disk[0].challenges]
            for what, pairs in (("meet_files", one), ("meet_one", many)):
                index = {id(b): i for i, b in enumerate(on_disk)}
                dpairs = [(on_dev[index[id(b)]], c) for b, c in pairs]
                arms = {"loop": forced("host", lambda: [b.meet_challenge(c) for b, c in pairs]),
                        "batch_host": forced("device", lambda: OneHash.meet_many(pairs)),
                        "batch_dev": forced("device", lambda: OneHash.meet_many(dpairs))}
                row = {"what": what, "files": len({id(b) for b, _ in pairs}), "jobs": len(pairs),
                       "file_bytes": MIB, "rounds": rounds}
                row.update(compare(rounds, arms))
                emit(row)

            # the job count from which a call is worth the GPU
            beat, pool = on_disk[0], list(on_disk[0].challenges)
            for jobs in (1, 4, 16, 32, 64, 128, 256, 512, 1024, 4096):
                chals = [Challenge(c.block, c.seed) for c in pool[:jobs]]
                row = {"what": "crossover_jobs", "jobs": jobs}
                for name, call in (("meet", lambda: beat.meet_challenges(chals)),
                                   ("generate", lambda: beat.generate_challenges(jobs, roots[0]))):
                    res = {}
                    for path in ("host", "device"):
                        f = forced(path, call)
                        f()
                        res[path] = stats([clock(f)[0] for _ in range(rounds + 2)])
                    row[name] = dict(res, device_faster=res["device"]["max_ms"] < res["host"]["min_ms"])
                emit(row)

            # host chain against device chain: small files, so that the chain is most of the call
            for k in (1, 4, 16, 64, 256):
                k = min(k, nfiles)
                small = [OneHash.from_device(dev + i * MIB, 4096, SECRET) for i in range(k)]
                items = [(b, 1000, r) for b, r in zip(small, roots)]
                res = {}
                for chain in ("host", "device"):
                    f = forced("device", lambda: OneHash.generate_challenges_many(items, chain=chain))
                    f()
                    res[chain] = stats([clock(f)[0] for _ in range(rounds + 2)])
                emit({"what": "chain", "files": k, "num": 1000, "host": res["host"], "device": res["device"],
                      "device_faster": res["device"]["max_ms"] < res["host"]["min_ms"]})
        finally:
            for b in on_disk:
                b.file_object.close()
            ctx.check(L.hb_device_free(ctx.h, dev))
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
