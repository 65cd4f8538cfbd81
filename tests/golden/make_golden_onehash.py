#!/usr/bin/env python3
"""Golden vectors of the OneHash scheme from the REFERENCE
(heartbeat/OneHash/OneHash.py): meet_challenge and generate_challenges.

Runs only where the reference checkout is (make_golden_merkle.py's REF).
Imports the unmodified reference modules heartbeat/exc.py and the
heartbeat/OneHash package under a synthetic ``heartbeat`` package; OneHash.py
needs only hashlib and random.

Output: onehash_cases.json next to this script (inputs and outputs only).

"meet": per file and block, the length of the file part the reference hashes
and its response for every seed length ("!Type: text" where it raises).  Blocks
cover both ends of the file, the first wrapped block, both sides of the point
from which the reference's first read comes up short, and what only a foreign
challenger sends: file_size, file_size + 1, file_size + 2 and -1.  Seed
lengths 0, 1, 31, 32, 33, 64, 65 and 100, plus those that put file part + seed
at 55, 56, 63 and 64 mod 64 (the padding's corners).

"generate": per case the blocks, seeds and responses of generate_challenges
and the value of random.random() drawn right after it -- the module-level
generator's state is part of the behaviour -- or the exception it raises.
Lists of more than 64 entries are held as the SHA-256 of their canonical JSON
and a few positions (tests/onehash_golden.py).
"""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_merkle import REF  # noqa: E402
from onehash_golden import det_bytes, file_bytes, pack, seed_of, write_files  # noqa: E402

SIZES = (0, 1, 9, 10, 11, 20, 100, 1000, 10239, 10240, 10241, 100003)
SEED_LENS = (0, 1, 31, 32, 33, 64, 65, 100)


def load_reference():
    pkg = types.ModuleType("heartbeat")
    pkg.__path__ = [os.path.join(REF, "heartbeat")]
    sys.modules["heartbeat"] = pkg

    def load(name, path, is_pkg=False):
        kw = {"submodule_search_locations": [os.path.dirname(path)]} if is_pkg else {}
        spec = importlib.util.spec_from_file_location(name, path, **kw)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("heartbeat.exc", os.path.join(REF, "heartbeat/exc.py"))
    return load("heartbeat.OneHash", os.path.join(REF, "heartbeat/OneHash/__init__.py"), True)


def blocks_of(fs):
    c = min(1024, fs // 10)
    inside = [0, 1, 2, 3, fs - c - 1, fs - c, fs - c + 1, fs - c + c // 2, fs - c + c // 2 + 1, fs - 2, fs - 1]
    seen = []
    for b in inside:
        if 0 <= b < fs and b not in seen:
            seen.append(b)
    return seen + [fs, fs + 1, fs + 2, -1]


def part_len(fs, block):
    """Bytes of the file in the message of an in-range block."""
    c = min(1024, fs // 10)
    if block <= fs - c:
        return c
    a = block - (fs - c)
    return min(a, c - a) + (c - a)


def outcome(fn):
    try:
        return fn()
    except Exception as e:   # recorded, whatever the reference does
        return "!%s: %s" % (type(e).__name__, e)


def main():
    M = load_reference()
    names = ["det%d" % n for n in SIZES] + ["test.txt"]
    meet, generate = [], []
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_files(tmp, names)
        for name in names:
            fs = len(file_bytes(name))
            beat = M.OneHash(paths[name])
            for block in blocks_of(fs):
                lens = list(SEED_LENS)
                plen = part_len(fs, block) if 0 <= block < fs else None
                if plen is not None:
                    lens += [x for x in sorted({(r - plen) % 64 for r in (55, 56, 63, 0)}) if x not in lens]

                def answer(sl):
                    r = beat.meet_challenge(M.Challenge(block, seed_of(sl)))
                    return r.hex()
                meet.append({"file": name, "block": block, "part_len": plen,
                             "answers": {str(sl): outcome(lambda: answer(sl)) for sl in lens}})

        def gen_case(name, num, root, secret):
            case = {"file": name, "num": num, "root_seed": root, "secret": None if secret is None else secret.hex()}
            t, v = root["t"], root["v"]
            root_seed = bytes.fromhex(v) if t == "bytes" else v
            beat = M.OneHash(paths[name], secret)
            random.seed("before-" + name)   # a known state, should the call fail before it seeds
            try:
                beat.generate_challenges(num, root_seed)
            except Exception as e:
                case["error"] = "!%s: %s" % (type(e).__name__, e)
            else:
                case["blocks"] = pack([c.block for c in beat.challenges])
                case["seeds"] = pack([c.seed.hex() for c in beat.challenges])
                case["responses"] = pack([c.response.hex() for c in beat.challenges])
            case["next_random"] = random.random()
            generate.append(case)

        root_bytes = {"t": "bytes", "v": det_bytes("onehash-root", 32).hex()}
        roots = [root_bytes, {"t": "str", "v": "a root seed"}, {"t": "int", "v": 1234567}, {"t": "float", "v": 1234.5}]
        secrets = [det_bytes("onehash-secret-%d" % n, n) for n in (0, 8, 23, 24, 87, 88, 200)] + [None]
        for name in ("det100003", "test.txt"):
            for secret in secrets:
                for num in (3, 300):
                    gen_case(name, num, root_bytes, secret)
            for root in roots:
                for num in (0, 1, 3, 300):
                    gen_case(name, num, root, secrets[1])
        for name in names:
            for num in (0, 3):
                gen_case(name, num, root_bytes, secrets[1])
    out = {"generator": "tests/golden/make_golden_onehash.py",
           "reference": "heartbeat/OneHash/OneHash.py",
           "files": {n: {"len": len(file_bytes(n))} for n in names}}
    with open(os.path.join(HERE, "onehash_cases.json"), "w") as f:
        # a case per line
        head = json.dumps(out, sort_keys=True, separators=(",", ":"))
        f.write(head[:-1])
        for key, cases in (("meet", meet), ("generate", generate)):
            f.write(',"%s":[\n' % key + ",\n".join(
                json.dumps(c, sort_keys=True, separators=(",", ":")) for c in cases) + "\n]")
        f.write("}\n")
    print("wrote %d meet and %d generate cases" % (len(meet), len(generate)))


if __name__ == "__main__":
    main()
