"""Merkle encode and prove: the batched calls against loops.

The shape: 256 files of 1 MiB, n = 256 challenges, chunks of 8192 bytes,
device-resident (DeviceFile) and from host memory (BytesIO).  After a warm-up
of every arm and a check that all arms give the same tags, `rounds`
alternating rounds of

  batch   one Merkle.encode_many over the files (hb_merkle_encode_many);
  loop_a  a loop of this build's Merkle.encode, one call per file;
  loop_b  the route before hb_merkle_encode_many existed: per file
          MerkleHelper.seed_chain (256 hmac calls), the leaves by
          device_chunk_hashes (two launches, two synchronising copies) or, for
          a host file, get_chunk_hashes, and a hashlib tree (MerkleTree.build);

each timed with a host clock around calls that return synchronised.  Then the
three kernels' times of a device-resident batch with the chain on the GPU
(hb_last_kernel_phases: chain, leaves, trees, copies back), the chain on the
host and on the GPU at 1, 4, 16, 64 and 256 small files (where the chain is
most of the call), from which MK_CHAIN_DEVICE_MIN_FILES (hb_merkle_host.hpp)
is taken, and Merkle.prove_many of 256 proofs against a loop of Merkle.prove.

  python scripts/merkle_rate.py [--rounds 5] [--files 256] [--out FILE]
"""
import ctypes
import hashlib
import importlib
import io
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402

MIB = 1 << 20
N, CHUNK = 256, 8192


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
            "spread_ms": round((max(ts) - min(ts)) * 1e3, 3)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


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


def compare(rounds, arms):
    """arms: name -> callable returning the tags' roots.  Warm-up, equality,
    then alternating rounds."""
    first = {k: f() for k, f in arms.items()}
    ref = first["batch"]
    for k, v in first.items():
        if v != ref or len(set(v)) != len(v):
            raise SystemExit("arm %s differs from the batch" % k)
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ts[k].append(clock(f)[0])
    row = {k: stats(v) for k, v in ts.items()}
    for k in arms:
        if k != "batch":
            row["batch_slowest_beats_%s_fastest" % k] = max(ts["batch"]) < min(ts[k])
            row["ratio_min_%s_over_max_batch" % k] = round(min(ts[k]) / max(ts["batch"]), 2)
            # the gain against the spread of the loop's own repeated timings
            row["gain_over_%s_spread" % k] = round((min(ts[k]) - max(ts["batch"])) /
                                                   max(max(ts[k]) - min(ts[k]), 1e-9), 1)
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
    M = importlib.import_module("heartbeat_amd.Merkle.Merkle")
    H, Tree = M.MerkleHelper, M.MerkleTree
    ctx = nat.context()
    key = hashlib.sha256(b"merkle-rate-key").digest()
    seeds = [hashlib.sha256(b"merkle-rate-seed/%d" % i).digest() for i in range(nfiles)]
    beat = M.Merkle(None, key)
    dev = Dev(ctx, nfiles * MIB, 0x5EED0400)
    rows = []
    try:
        host = dev.download()
        hostb = [host[i * MIB:(i + 1) * MIB].tobytes() for i in range(nfiles)]
        dfiles = [M.DeviceFile(dev.p + i * MIB, MIB) for i in range(nfiles)]

        def parent_route(i, where):
            chain = H.seed_chain(key, seeds[i], N)
            if where == "dev":
                _, leaves = H.device_chunk_hashes(dev.p + i * MIB, MIB, chain, None, CHUNK)
            else:
                leaves = H.get_chunk_hashes(io.BytesIO(hostb[i]), chain, None, CHUNK)
            t = Tree()
            for leaf in leaves:
                t.add_leaf(leaf)
            t.build()
            return t.get_root()

        for where in ("dev", "host"):
            files = (lambda: dfiles) if where == "dev" else (lambda: [io.BytesIO(b) for b in hostb])
            arms = {
                "batch": lambda: [s.root for _, s in beat.encode_many(files(), N, seeds, CHUNK)],
                "loop_a": lambda: [beat.encode(f, N, s, CHUNK)[1].root for f, s in zip(files(), seeds)],
                "loop_b": lambda: [parent_route(i, where) for i in range(nfiles)],
            }
            row = {"what": "encode", "files": nfiles, "file_bytes": MIB, "n": N, "chunksz": CHUNK, "where": where,
                   "rounds": rounds, "build": nat.build_info()["build_id"]}
            row.update(compare(rounds, arms))
            print(json.dumps(row), flush=True)
            rows.append(row)

        # the three kernels of a device-resident batch, the chain on the GPU
        ph = []
        for _ in range(rounds):
            M.encode_batch([(beat, f, N, s, CHUNK, None) for f, s in zip(dfiles, seeds)], chain="device")
            ph.append(ctx.last_kernel_phases())
        names = ("chain_ms", "leaves_ms", "trees_ms", "copies_back_ms")
        row = {"what": "kernels", "files": nfiles, "where": "dev", "rounds": rounds}
        row.update({nm: {"min": min(p[k] for p in ph), "max": max(p[k] for p in ph)} for k, nm in enumerate(names)})
        print(json.dumps(row), flush=True)
        rows.append(row)

        # host chain against device chain: small files, so that the chain is most of the call
        for k in (1, 4, 16, 64, 256):
            k = min(k, nfiles)
            small = [M.DeviceFile(dev.p + i * MIB, 4096) for i in range(k)]
            items = [(beat, f, N, s, 64, None) for f, s in zip(small, seeds)]
            res = {}
            for chain in ("host", "device"):
                M.encode_batch(items, chain=chain)
                ts, p0 = [], []
                for _ in range(rounds + 2):
                    ts.append(clock(lambda: M.encode_batch(items, chain=chain))[0])
                    p0.append(ctx.last_kernel_phases()[0])
                res[chain] = dict(stats(ts), first_phase_ms_min=min(p0))
            row = {"what": "chain", "files": k, "n": N, "host": res["host"], "device": res["device"],
                   "device_faster": res["device"]["max_ms"] < res["host"]["min_ms"]}
            print(json.dumps(row), flush=True)
            rows.append(row)

        # prove_many against a loop of prove
        for where in ("dev", "host"):
            files = (lambda: dfiles) if where == "dev" else (lambda: [io.BytesIO(b) for b in hostb])
            tags_states = beat.encode_many(files(), N, seeds, CHUNK)
            chals = [beat.gen_challenge(s) for _, s in tags_states]
            tags = [t for t, _ in tags_states]
            pub = beat.get_public()
            arms = {
                "batch": lambda: [p.leaf.blob for p in M.Merkle.prove_many(list(zip(files(), chals, tags)))],
                "loop": lambda: [pub.prove(f, c, t).leaf.blob for f, c, t in zip(files(), chals, tags)],
            }
            row = {"what": "prove", "proofs": nfiles, "where": where, "rounds": rounds}
            row.update(compare(rounds, arms))
            ok = all(beat.verify(p, c, s) for p, c, (_, s) in
                     zip(M.Merkle.prove_many(list(zip(files(), chals, tags))), chals, tags_states))
            row["proofs_verify"] = ok
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        dev.free()
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
