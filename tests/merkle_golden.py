"""Reading tests/golden/merkle_scheme_cases.json.

Cases of up to FULL_MAX_N leaves hold everything the reference returned in
full.  For the larger ones (n = 64, 65, 256, 257: a quarter of a megabyte of
base64 each) the lists are held as the SHA-256 of their canonical JSON, which
pins every element just the same, and in full at SAMPLE positions only.  The
functions here compare a result with a case in either form."""
import base64
import hashlib
import hmac
import json

FULL_MAX_N = 9


def canon(x):
    """The canonical JSON text of a todict() result (tuples become lists)."""
    return json.dumps(x, sort_keys=True, separators=(",", ":"))


def digest(x):
    return hashlib.sha256(canon(x).encode()).hexdigest()


def plain(x):
    """A todict() as JSON holds it."""
    return json.loads(canon(x))


def samples(n):
    """The positions a large case holds in full."""
    return sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n)))


def file_bytes(name):
    from test_oracle import _merkle_file
    return b"" if name == "empty" else _merkle_file(name)


def tag_matches(c, d):
    d, want = plain(d), c["tag"]
    if "tree" in want:
        return d == want
    return ((d["chunksz"], d["filesz"], d["tree"]["order"], d["tree"]["leaves"]) ==
            (want["chunksz"], want["filesz"], want["order"], []) and digest(d["tree"]) == want["tree_sha256"])


def _list_matches(c, name, got):
    got = plain(got)
    if name in c:
        return got == c[name]
    return (len(got) == c["n"] and digest(got) == c[name + "_sha256"] and
            all(got[int(i)] == v for i, v in c[name + "_at"].items()))


def leaves_match(c, hex_leaves):
    return _list_matches(c, "leaves", list(hex_leaves))


def challenges_match(c, dicts):
    return _list_matches(c, "challenges", list(dicts))


def proofs_match(c, dicts):
    return _list_matches(c, "proofs", list(dicts))


def sampled(c, name):
    """{position: element} of a case's list: every position of a small case."""
    if name in c:
        return dict(enumerate(c[name]))
    return {int(i): v for i, v in c[name + "_at"].items()}


def chain(c):
    """The case's n leaf seeds (Merkle.py:357-361), by hmac."""
    key, s, out = bytes.fromhex(c["key"]), bytes.fromhex(c["seed"]), []
    for _ in range(c["n"]):
        s = hmac.new(key, s, hashlib.sha256).digest()
        out.append(s)
    return out


def leaves_of(c, oracle):
    """The case's leaf blobs: recorded, or for a large case restated with the
    oracle (and then checked against the recorded digest)."""
    if "leaves" in c:
        return [bytes.fromhex(x) for x in c["leaves"]]
    data = file_bytes(c["file"])
    out = [oracle.merkle_chunk_hash(data, s, c["tag"]["filesz"], c["tag"]["chunksz"]) for s in chain(c)]
    assert leaves_match(c, [x.hex() for x in out])
    return out


def b64(x):
    return base64.b64decode(x)
