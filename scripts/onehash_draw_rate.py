"""OneHash: the positions of a GPU generate call drawn on the device against
pick_blocks (OH_DRAW_DEVICE_MIN_JOBS in hb_onehash_host.hpp).

Three arms run the same public call with the GPU path forced
(HB_ONEHASH_DEVICE=1), each in a process of its own that keeps its context:

  parent   the parent commit's tree (--parent DIR: a checkout with its own
           built library), the baseline: pick_blocks in a Python loop
  host     this tree with draw="host": must agree with the parent
  device   this tree with draw="device": hb_onehash_generate_drawn_many

Every arm is warmed up and must give the same blocks, seeds and responses;
then `rounds` alternating rounds, each call timed by its own process with a
host clock around a call that returns synchronised.  min ... max in ms are
reported, and whether the device draw's slowest round beats the parent's
fastest.  Shapes, each from files on disk and device-resident:

  gen_one    generate_challenges(10000) on one 1 MiB file
  gen_many   generate_challenges_many of 256 files x 1000
  gen_16     generate_challenges_many of 16 files x 1000
  sweep      generate_challenges of 256, 512, 1024, 4096 on one 1 MiB file

  python scripts/onehash_draw_rate.py --parent DIR [--rounds 5] [--files 256]
         [--out profiles/many/onehash_draw_rate.json]
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

MIB = 1 << 20
SECRET = b"mysecret"
SHAPES = [("gen_one", 1, 10000), ("gen_many", 256, 1000), ("gen_16", 16, 1000),
          ("sweep", 1, 256), ("sweep", 1, 512), ("sweep", 1, 1024), ("sweep", 1, 4096)]


# ---------------------------------------------------------------- one arm's process
def worker(tree, draw, files_dir, nfiles):
    """Serves "<where> <files> <num>" lines on stdin: runs the call once and
    answers "<seconds> <sha256 of the challenges>"."""
    sys.path.insert(0, tree)
    os.environ["HB_ONEHASH_DEVICE"] = "1"
    import numpy as np
    from heartbeat_amd import _native as nat
    from heartbeat_amd.OneHash import OneHash
    ctx, L = nat.context(), nat.lib()
    p = ctypes.c_void_p()
    ctx.check(L.hb_device_malloc(ctx.h, nfiles * MIB, ctypes.byref(p)))
    paths = [os.path.join(files_dir, "f%d.bin" % i) for i in range(nfiles)]
    for i, q in enumerate(paths):
        data = np.fromfile(q, dtype=np.uint8)
        ctx.check(L.hb_memcpy(ctx.h, p.value + i * MIB, data.ctypes.data, MIB, 1))
    beats = {"disk": [OneHash(q, SECRET) for q in paths],
             "resident": [OneHash.from_device(p.value + i * MIB, MIB, SECRET) for i in range(nfiles)]}
    roots = [hashlib.sha256(b"onehash-rate-root/%d" % i).digest() for i in range(nfiles)]
    kw = {} if draw == "none" else {"draw": draw}
    print("ready %s" % nat.build_info()["build_id"][:16], flush=True)
    for line in sys.stdin:
        where, k, num = line.split()
        k, num = int(k), int(num)
        items = [(b, num, r) for b, r in zip(beats[where][:k], roots)]
        t0 = time.perf_counter()
        OneHash.generate_challenges_many(items, **kw)
        dt = time.perf_counter() - t0
        h = hashlib.sha256()
        for b, _, _ in items:
            for c in b.challenges:
                h.update(b"%d|" % c.block + c.seed + c.response)
        print("%.9f %s" % (dt, h.hexdigest()), flush=True)


class Arm(object):
    def __init__(self, tree, draw, files_dir, nfiles):
        env = dict(os.environ, PYTHONPATH=tree)
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, draw, files_dir,
                                      str(nfiles)], cwd=tree, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True)
        self.build = self._line().split()[1]

    def _line(self):
        line = self.proc.stdout.readline()
        if not line:
            raise SystemExit("an arm's process ended: exit status %s" % self.proc.wait())
        return line

    def run(self, where, k, num):
        self.proc.stdin.write("%s %d %d\n" % (where, k, num))
        self.proc.stdin.flush()
        dt, digest = self._line().split()
        return float(dt), digest

    def close(self):
        self.proc.stdin.close()
        self.proc.wait()


def stats(ts):
    return {"min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def main(argv):
    if argv[:1] == ["--worker"]:
        return worker(argv[1], argv[2], argv[3], int(argv[4]))
    rounds, out, nfiles, parent = 5, None, 256, None
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--out":
            out = next(it)
        elif x == "--files":
            nfiles = int(next(it))
        elif x == "--parent":
            parent = os.path.abspath(next(it))
    if parent is None:
        raise SystemExit(__doc__)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(nfiles):
            with open(os.path.join(tmp, "f%d.bin" % i), "wb") as fh:
                fh.write(hashlib.shake_128(b"onehash-draw-rate/%d" % i).digest(MIB))
        arms = {"parent": Arm(parent, "none", tmp, nfiles), "host": Arm(here, "host", tmp, nfiles),
                "device": Arm(here, "device", tmp, nfiles)}
        try:
            for what, k, num in SHAPES:
                k = min(k, nfiles)
                for where in ("disk", "resident"):
                    first = {name: arm.run(where, k, num)[1] for name, arm in arms.items()}   # warm-up
                    if len(set(first.values())) != 1:
                        raise SystemExit("%s %s: the arms differ: %s" % (what, where, first))
                    ts = {name: [] for name in arms}
                    for _ in range(rounds):
                        for name, arm in arms.items():
                            ts[name].append(arm.run(where, k, num)[0])
                    row = {"what": what, "where": where, "files": k, "num": num, "jobs": k * num, "rounds": rounds,
                           "file_bytes": MIB, "builds": {name: arm.build for name, arm in arms.items()}}
                    row.update({name: stats(v) for name, v in ts.items()})
                    row["device_slowest_beats_parent_fastest"] = max(ts["device"]) < min(ts["parent"])
                    row["ratio_min_parent_over_max_device"] = round(min(ts["parent"]) / max(ts["device"]), 2)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
        finally:
            for arm in arms.values():
                arm.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
