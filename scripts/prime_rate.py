"""getPrimes on the GPU against the host loop it replaces.

For bits in 256, 512, 1024, 2048 and count in 1, 16, 256 one row each:

  gpu       wall time of getPrimes(bits, count) (host clock around the call:
            drawing starts and bases from os.urandom, the sieve, every test
            launch and the copies), the fastest and slowest of --rounds calls
            after one warm-up call per size (code object load), and of the
            fastest call its launches and lane tests (hb_prime_search's
            tests_out);
  host      the parent's path on the same box: the mean of timed getPrime(bits)
            draws (--host-draws at <= 1024 bits, --host-draws-2048 at 2048)
            times count -- a loop of count constructors;
  ratio     host / gpu (slowest gpu call).

  python scripts/prime_rate.py [--rounds 3] [--host-draws 8] [--host-draws-2048 2] [--out FILE]

Every prime drawn is checked for its bit length; the GPU tests
(tests/test_gpu_getprimes.py) check primality with the host Miller-Rabin.
"""
import json
import sys
import time

sys.path.insert(0, ".")
from heartbeat_amd import _native as nat   # noqa: E402
from heartbeat_amd import primes           # noqa: E402
from heartbeat_amd.PySwizzle.PySwizzle import getPrime   # noqa: E402

BITS = (256, 512, 1024, 2048)
COUNTS = (1, 16, 256)


def host_mean_s(bits, draws):
    t = []
    for _ in range(draws):
        t0 = time.perf_counter()
        p = getPrime(bits)
        t.append(time.perf_counter() - t0)
        assert p.bit_length() == bits
    return sum(t) / len(t), t


def gpu_row(bits, count, rounds):
    best = None
    times = []
    for _ in range(rounds):
        stats = {}
        t0 = time.perf_counter()
        ps = primes.getPrimes(bits, count, stats=stats)
        dt = time.perf_counter() - t0
        assert len(ps) == count and all(p.bit_length() == bits and p & 1 for p in ps)
        times.append(dt)
        if best is None or dt < best[0]:
            best = (dt, stats)
    return {"min_ms": round(1e3 * min(times), 3), "max_ms": round(1e3 * max(times), 3), "rounds": rounds,
            "launches": best[1]["launches"], "tests": best[1]["tests"]}


def main(argv):
    rounds, draws, draws2048, out = 3, 8, 2, "profiles/many/prime_rate.json"
    it = iter(argv)
    for x in it:
        if x == "--rounds":
            rounds = int(next(it))
        elif x == "--host-draws":
            draws = int(next(it))
        elif x == "--host-draws-2048":
            draws2048 = int(next(it))
        elif x == "--out":
            out = next(it)
        else:
            raise SystemExit("unknown argument %s" % x)
    if draws < 8 or draws2048 < 2:
        raise SystemExit("at least 8 host draws at <= 1024 bits and 2 at 2048")
    build = nat.build_info()["build_id"]
    rows = []
    for bits in BITS:
        n = draws2048 if bits == 2048 else draws
        mean_s, each = host_mean_s(bits, n)
        primes.getPrimes(bits, 2)   # warm-up: the class's code object
        for count in COUNTS:
            g = gpu_row(bits, count, rounds)
            row = {"what": "getPrimes", "bits": bits, "count": count, "rounds_mr": 40, "window": 4 * bits,
                   "build": build, "gpu": g,
                   "host": {"mean_ms_per_prime": round(1e3 * mean_s, 3), "draws": n,
                            "min_ms": round(1e3 * min(each), 3), "max_ms": round(1e3 * max(each), 3),
                            "loop_ms": round(1e3 * mean_s * count, 3)},
                   "ratio_host_loop_over_gpu_max": round(mean_s * count / (g["max_ms"] / 1e3), 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            with open(out, "w") as fh:   # after every row: a long run leaves what it has
                json.dump(rows, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
