"""Reading tests/golden/onehash_cases.json: the files the recorder used, the
seeds and root seeds as the JSON holds them, and the comparison of a list with
a case that holds it in full or (above FULL_MAX entries) as the SHA-256 of its
canonical JSON plus a few positions."""
import hashlib
import os

from merkle_golden import digest, samples

FULL_MAX = 64
HERE = os.path.dirname(os.path.abspath(__file__))


def det_bytes(tag, n):
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(("%s/%d" % (tag, i)).encode()).digest()
        i += 1
    return out[:n]


def file_bytes(name):
    """The bytes of a golden file: "test.txt", or "det<size>"."""
    if name == "test.txt":
        with open(os.path.join(HERE, "golden", "files", "test.txt"), "rb") as fh:
            return fh.read()
    return det_bytes("onehash-file-%s" % name[3:], int(name[3:]))


def seed_of(length):
    """The seed of `length` bytes of the meet cases."""
    return det_bytes("onehash-seed-%d" % length, length)


def root_seed_of(d):
    """A root seed from its JSON form {"t": type name, "v": value}."""
    return {"bytes": bytes.fromhex, "str": str, "int": int, "float": float}[d["t"]](d["v"])


def pack(xs):
    """A list as a case holds it."""
    xs = list(xs)
    if len(xs) <= FULL_MAX:
        return {"all": xs}
    return {"n": len(xs), "sha256": digest(xs), "at": {str(i): xs[i] for i in samples(len(xs))}}


def matches(packed, xs):
    xs = list(xs)
    if "all" in packed:
        return xs == packed["all"]
    return (len(xs) == packed["n"] and digest(xs) == packed["sha256"] and
            all(xs[int(i)] == v for i, v in packed["at"].items()))


def write_files(directory, names):
    """The golden files as real files under `directory`: {name: path}."""
    out = {}
    for name in names:
        path = os.path.join(str(directory), name + ".bin")
        with open(path, "wb") as fh:
            fh.write(file_bytes(name))
        out[name] = path
    return out
