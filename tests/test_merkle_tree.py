"""The host side of the Merkle scheme (heartbeat_amd/Merkle: MerkleTree.py and
the containers, gen_challenge and verify of Merkle.py) against the reference's
recorded outputs (tests/golden/merkle_scheme_cases.json, read through
tests/merkle_golden.py).  No GPU: encode and prove are in
tests/test_gpu_merkle_scheme.py."""
import copy
import importlib

import pytest

import merkle_golden as mg
from conftest import load_golden

G = load_golden("merkle_scheme_cases.json")
CASES = G["cases"]
IDS = ["%s-n%d-c%s-%d" % (c["file"], c["n"], c["chunksz"], i) for i, c in enumerate(CASES)]
SMALL = [c for c in CASES if c["n"] <= mg.FULL_MAX_N]


@pytest.fixture(scope="module")
def M():
    # the package attribute `Merkle` is the class, as in the reference
    return importlib.import_module("heartbeat_amd.Merkle.Merkle")


def _tree(c, oracle):
    from heartbeat_amd.Merkle import MerkleTree
    t = MerkleTree()
    for leaf in mg.leaves_of(c, oracle):
        t.add_leaf(leaf)
    t.build()
    return t


def _flip(b, at=0):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def test_golden_covers_the_issue_cases():
    assert {c["n"] for c in CASES} >= {1, 2, 3, 5, 8, 9, 64, 65, 256, 257}
    big = G["files"]["rand100k"]["len"]
    assert {c["chunksz"] for c in CASES} >= {8192, 100, 1, big, big + 10}
    assert any(c["check_fraction"] is not None for c in CASES)
    assert any(c["filesz"] is not None for c in CASES)
    assert {len(c["key"]) // 2 for c in CASES} >= {16, 32, 70}
    assert {len(c["seed"]) // 2 for c in CASES} >= {5, 32}
    assert any(c["file"] == "empty" for c in CASES) and not any("error" in c for c in CASES)
    assert all(len(c["verdicts"]) == c["n"] and all(c["verdicts"]) and c["exhausted"] == "Out of challenges."
               for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_tree_nodes_root_and_branches(c, M, oracle):
    t = _tree(c, oracle)
    blobs = [leaf.blob for leaf in t.leaves]
    proofs = [{"leaf": M.MerkleLeaf(i, blobs[i]).todict(), "branch": t.get_branch(i).todict()}
              for i in range(c["n"])]
    assert mg.proofs_match(c, proofs)                    # get_branch(i) for every i
    assert t.get_root() == mg.b64(c["state"]["root"])
    nodes = list(t.nodes)
    assert len(nodes) == 2 << t.order
    # empty: the leaf slots >= n and the unused last entry, nothing else
    assert [k for k, x in enumerate(nodes) if not x] == list(range((1 << t.order) - 1 + c["n"], 2 << t.order))
    # the same from a raw node buffer, as a GPU encode hands it over
    r = M.MerkleTree._from_raw(b"".join(x if x else bytes(32) for x in nodes), t.order, c["n"])
    assert r.get_root() == t.get_root()
    assert [r.get_branch(i).todict() for i in range(c["n"])] == [p["branch"] for p in proofs]
    assert r._raw is not None                            # nothing materialised by root and branches
    t.strip_leaves()
    assert r == t and r._raw is None
    # the nodes, which slots are b'' included: the reference's stripped tree
    assert mg.tag_matches(c, {"tree": r.todict(), "chunksz": c["tag"]["chunksz"], "filesz": c["tag"]["filesz"]})
    assert M.MerkleTree.fromdict(mg.plain(t.todict())) == t


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_verify_branch(c, M):
    from heartbeat_amd.Merkle.MerkleTree import MerkleBranch, MerkleLeaf, MerkleTree
    root = mg.b64(c["state"]["root"])
    for i, p in mg.sampled(c, "proofs").items():
        if i not in mg.samples(c["n"]):
            continue
        leaf, branch = MerkleLeaf.fromdict(p["leaf"]), MerkleBranch.fromdict(p["branch"])
        assert leaf.index == i and MerkleTree.verify_branch(leaf, branch, root)
        assert not MerkleTree.verify_branch(MerkleLeaf(leaf.index, _flip(leaf.blob, 31)), branch, root)
        assert not MerkleTree.verify_branch(MerkleLeaf(leaf.index + 1, leaf.blob), branch, root)
        assert not MerkleTree.verify_branch(leaf, branch, _flip(root, 7))
        for row in range(branch.get_order()):
            for side in (0, 1):
                if not branch.rows[row][side]:
                    continue
                bad = copy.deepcopy(branch)
                pair = list(bad.rows[row])
                pair[side] = _flip(pair[side], 5)
                bad.set_row(row, tuple(pair))
                assert not MerkleTree.verify_branch(leaf, bad, root)
    # a leaf that cannot be hashed is a failed proof, not an error
    assert not MerkleTree.verify_branch(MerkleLeaf(0, None), MerkleBranch(0), root)


def test_index_helpers_and_order(M):
    T = M.MerkleTree
    assert [T.get_parent(i) for i in (1, 2, 3, 4, 5, 6)] == [0, 0, 1, 1, 2, 2]
    assert [T.get_partner(i) for i in (1, 2, 3, 4)] == [2, 1, 4, 3]
    assert [T.is_left(i) for i in (1, 2, 3, 4)] == [True, False, True, False]
    assert (T.get_left_child(0), T.get_right_child(0), T.get_left_child(4), T.get_right_child(4)) == (1, 2, 9, 10)
    assert [T.get_order(n) for n in (1, 2, 3, 4, 5, 8, 9, 256, 257, 65536)] == [0, 1, 2, 2, 3, 3, 4, 8, 9, 16]
    with pytest.raises(ValueError):
        T.get_order(0)


@pytest.mark.parametrize("c", [SMALL[3], SMALL[5], SMALL[-1]], ids=["n5", "n9", "empty"])
def test_containers_round_trip(c, M):
    tag = M.Tag.fromdict(c["tag"])
    assert tag.todict() == c["tag"] and M.Tag.fromdict(tag.todict()) == tag
    assert tag.tree.todict() == c["tag"]["tree"] and M.MerkleTree.fromdict(tag.tree.todict()) == tag.tree
    state = M.State.fromdict(c["state"])
    assert state.todict() == c["state"] and M.State.fromdict(state.todict()) == state
    for ch, pr in zip(c["challenges"], c["proofs"]):
        chal, proof = M.Challenge.fromdict(ch), M.Proof.fromdict(pr)
        assert chal.todict() == ch and M.Challenge.fromdict(chal.todict()) == chal
        assert mg.plain(proof.todict()) == pr and M.Proof.fromdict(proof.todict()) == proof
        assert proof.leaf.todict() == pr["leaf"] and mg.plain(proof.branch.todict()) == pr["branch"]
    beat = M.Merkle(c["check_fraction"], bytes.fromhex(c["key"]))
    again = M.Merkle.fromdict(beat.todict())
    assert again == beat and again.check_fraction == c["check_fraction"]
    pub = beat.get_public()
    assert pub.key == b"" and pub.check_fraction == c["check_fraction"]
    assert (M.Merkle.tag_type(), M.Merkle.state_type(), M.Merkle.challenge_type(), M.Merkle.proof_type()) == (
        M.Tag, M.State, M.Challenge, M.Proof)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_state_hmac_and_gen_challenge(c, M):
    key = bytes.fromhex(c["key"])
    beat = M.Merkle(c["check_fraction"], key)
    state = M.State.fromdict(c["state"])
    assert state.timestamp == G["timestamp"]
    assert state.get_hmac(key) == mg.b64(c["state"]["hmac"])
    state.checksig(key)
    fresh = M.State(0, bytes.fromhex(c["seed"]), c["n"], mg.b64(c["state"]["root"]), None, G["timestamp"])
    fresh.sign(key)
    assert fresh == state
    assert mg.challenges_match(c, [beat.gen_challenge(state).todict() for _ in range(c["n"])])
    assert state.todict() == c["state_after"]          # signed again after every challenge
    with pytest.raises(M.HeartbeatError, match="Out of challenges."):
        beat.gen_challenge(state)
    for field, bad in (("index", 1), ("seed", _flip(state.seed)), ("n", state.n + 1),
                       ("root", _flip(state.root)), ("timestamp", state.timestamp + 1)):
        t = M.State.fromdict(c["state"])
        setattr(t, field, bad)
        with pytest.raises(M.HeartbeatError, match="Signature invalid on state."):
            beat.gen_challenge(t)
    with pytest.raises(M.HeartbeatError, match="Signature invalid on state."):
        M.Merkle(None, key + b"x").gen_challenge(M.State.fromdict(c["state"]))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_verify(c, M):
    key = bytes.fromhex(c["key"])
    beat = M.Merkle(c["check_fraction"], key)
    state = M.State.fromdict(c["state_after"])
    chals, proofs = mg.sampled(c, "challenges"), mg.sampled(c, "proofs")
    for i in mg.samples(c["n"]):
        chal, proof = M.Challenge.fromdict(chals[i]), M.Proof.fromdict(proofs[i])
        assert chal.index == i and beat.verify(proof, chal, state) is True
        assert beat.verify(proof, M.Challenge(chal.seed, chal.index + 1), state) is False   # index mismatch
        wrong = M.Proof(M.MerkleLeaf(proof.leaf.index, _flip(proof.leaf.blob)), proof.branch)
        assert beat.verify(wrong, chal, state) is False
    tampered = M.State.fromdict(c["state_after"])
    tampered.root = _flip(tampered.root)
    with pytest.raises(M.HeartbeatError, match="Signature invalid on state."):
        beat.verify(M.Proof.fromdict(proofs[0]), M.Challenge.fromdict(chals[0]), tampered)


def test_state_default_timestamp_is_fixed_at_import(M):
    """As the reference's: the default argument is evaluated once."""
    assert M.State().timestamp == M.State().timestamp


def test_encode_rejects_n_without_touching_the_gpu(M):
    import io
    for n in (0, -1, 65537):
        with pytest.raises(M.HeartbeatError, match="n must be in 1..65536"):
            M.Merkle(None, b"k" * 32).encode(io.BytesIO(b"data"), n)
    assert M.Merkle.encode_mixed([]) == [] and M.Merkle.prove_many([]) == []
    assert M.Merkle(None, b"k").encode_many([]) == []
