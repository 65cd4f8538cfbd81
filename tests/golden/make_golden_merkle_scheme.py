#!/usr/bin/env python3
"""Golden vectors of the whole Merkle scheme from the REFERENCE
(heartbeat/Merkle/Merkle.py, MerkleTree.py): Merkle.encode, gen_challenge,
prove and verify.

Runs only where the reference checkout is (make_golden_merkle.py's REF).
Imports the unmodified reference modules under a synthetic ``heartbeat``
package with the offline PyCrypto-API shim (tests/golden/shim), through
make_golden_merkle.py's loader.
The reference's State takes its default timestamp from time.time() when the
module is loaded, so the clock is pinned for that moment: the file
regenerates byte for byte.

Output: merkle_scheme_cases.json next to this script (inputs and outputs
only).  Per case: the tag, the leaf blobs before stripping, the signed state,
every challenge of the state's life, every proof and every verdict.  Cases of
more than FULL_MAX_N leaves hold the tree and the three lists as the SHA-256
of their canonical JSON (tests/merkle_golden.py), which pins every element,
and in full only at a few positions: in full they are a quarter of a megabyte
each.
"""
import io
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_merkle import det_bytes, load_reference  # noqa: E402
from merkle_golden import FULL_MAX_N, digest, plain, samples  # noqa: E402

TIMESTAMP = 1400000000.25


def load_pinned():
    real = time.time
    time.time = lambda: TIMESTAMP
    try:
        return load_reference()
    finally:
        time.time = real


def main():
    M = load_pinned()
    files = {
        "test.txt": open(os.path.join(HERE, "files", "test.txt"), "rb").read(),
        "rand100k": det_bytes("merkle-file", 100003),
        "tiny5": det_bytes("merkle-tiny", 5),
        "empty": b"",
    }
    key32 = det_bytes("merkle-scheme-key", 32)
    seed32 = det_bytes("merkle-scheme-seed", 32)
    big = len(files["rand100k"])
    # (file, key, seed, n, chunksz, filesz, check_fraction)
    specs = [("rand100k", key32, seed32, n, 8192, None, None) for n in (1, 2, 3, 5, 8, 9, 64, 65, 256, 257)]
    specs += [("rand100k", key32, seed32, 5, c, None, None) for c in (100, 1, big, big + 10)]
    specs += [
        ("test.txt", key32, seed32, 9, None, None, None),           # the default chunk size
        ("tiny5", key32, seed32, 3, 8192, None, None),              # the chunk clamps to the file
        ("tiny5", key32, seed32, 2, 1, None, None),
        ("rand100k", key32, seed32, 8, None, None, 0.01),           # check_fraction
        ("rand100k", key32, seed32, 5, 100, 50000, None),           # an explicit filesz < len
        ("rand100k", det_bytes("merkle-scheme-key16", 16), seed32, 5, 8192, None, None),
        ("rand100k", det_bytes("merkle-scheme-key70", 70), seed32, 5, 8192, None, None),
        ("rand100k", key32, det_bytes("merkle-scheme-seed5", 5), 5, 8192, None, None),
        ("empty", key32, seed32, 3, 8192, None, None),              # a zero-length file
    ]
    cases = []
    for fname, key, seed, n, chunksz, filesz, frac in specs:
        data = files[fname]
        case = {"file": fname, "key": key.hex(), "seed": seed.hex(), "n": n, "chunksz": chunksz,
                "filesz": filesz, "check_fraction": frac}
        beat = M.Merkle(frac, key)
        # the leaf blobs: encode strips them, so the chain is walked once more
        eff_filesz = len(data) if filesz is None else filesz
        eff_chunk = chunksz if chunksz is not None else (int(frac * eff_filesz) if frac is not None else 8192)
        try:
            f = io.BytesIO(data)
            tag, state = beat.encode(f, n, seed, chunksz, filesz)
        except Exception as e:   # recorded, whatever the reference does
            case["error"] = "%s: %s" % (type(e).__name__, e)
            cases.append(case)
            continue
        case["file_pos_after_encode"] = f.tell()
        s = seed
        leaves = []
        for _ in range(n):
            s = M.MerkleHelper.get_next_seed(key, s)
            leaves.append(M.MerkleHelper.get_chunk_hash(io.BytesIO(data), s, eff_filesz, eff_chunk).hex())
        case["leaves"] = leaves
        case["tag"] = tag.todict()
        case["state"] = state.todict()
        public = beat.get_public()
        chals, proofs, verdicts = [], [], []
        for _ in range(n):
            chal = beat.gen_challenge(state)
            proof = public.prove(io.BytesIO(data), chal, tag)
            chals.append(chal.todict())
            proofs.append(proof.todict())
            verdicts.append(bool(beat.verify(proof, chal, state)))
        case["challenges"] = chals
        case["proofs"] = proofs
        case["verdicts"] = verdicts
        case["state_after"] = state.todict()
        try:
            beat.gen_challenge(state)
            case["exhausted"] = None
        except Exception as e:
            case["exhausted"] = str(e)
        if n > FULL_MAX_N:
            tag = case["tag"]
            case["tag"] = {"chunksz": tag["chunksz"], "filesz": tag["filesz"], "order": tag["tree"]["order"],
                           "tree_sha256": digest(tag["tree"])}
            for name in ("leaves", "challenges", "proofs"):
                full = plain(case.pop(name))
                case[name + "_sha256"] = digest(full)
                case[name + "_at"] = {str(i): full[i] for i in samples(n)}
        cases.append(case)
    out = {"generator": "tests/golden/make_golden_merkle_scheme.py",
           "reference": "heartbeat/Merkle/Merkle.py, heartbeat/Merkle/MerkleTree.py",
           "timestamp": TIMESTAMP,
           "files": {k: {"len": len(v)} for k, v in files.items()},
           "cases": cases}
    with open(os.path.join(HERE, "merkle_scheme_cases.json"), "w") as f:
        # a case per line
        head = json.dumps({k: v for k, v in out.items() if k != "cases"}, sort_keys=True, separators=(",", ":"))
        f.write(head[:-1] + ',"cases":[\n' + ",\n".join(
            json.dumps(c, sort_keys=True, separators=(",", ":")) for c in cases) + "\n]}\n")
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
