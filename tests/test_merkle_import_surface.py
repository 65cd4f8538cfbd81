"""The Merkle scheme's surface: the reference package's names under
heartbeat_amd.Merkle in a fresh interpreter that never loads the native
library, the ctypes signatures beside the header, and the heartbeat/ alias
package unchanged (the scheme is reached as heartbeat_amd.Merkle)."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_names_import_without_the_native_library():
    code = (
        "import sys\n"
        "from heartbeat_amd.Merkle import (Challenge, Tag, State, Proof, Merkle, MerkleHelper, MerkleTree,\n"
        "                                  DEFAULT_CHUNK_SIZE, DeviceFile)\n"
        "from heartbeat_amd.Merkle.Merkle import MerkleHelper as H2, encode_batch, prove_batch\n"
        "from heartbeat_amd.Merkle.MerkleTree import MerkleLeaf, MerkleBranch\n"
        "from heartbeat_amd import _native\n"
        "assert H2 is MerkleHelper and DEFAULT_CHUNK_SIZE == 8192\n"
        "m = Merkle(0.5, b'k' * 32)\n"
        "assert Merkle.fromdict(m.todict()) == m and m.get_public().key == b''\n"
        "for name in ('encode', 'encode_many', 'encode_mixed', 'gen_challenge', 'prove', 'prove_many', 'verify',\n"
        "             'tag_type', 'state_type', 'challenge_type', 'proof_type'):\n"
        "    assert callable(getattr(Merkle, name)), name\n"
        "for name in ('add_leaf', 'build', 'get_branch', 'get_root', 'strip_leaves', 'get_parent', 'get_partner',\n"
        "             'is_left', 'get_left_child', 'get_right_child', 'get_order', 'verify_branch', 'todict',\n"
        "             'fromdict'):\n"
        "    assert callable(getattr(MerkleTree, name)), name\n"
        "assert _native._lib is None, 'importing the scheme loaded libhbswizzle.so'\n"
        "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_native_binding_lists_the_merkle_calls():
    from heartbeat_amd import _native
    sig = {s[0]: s for s in _native.SIGNATURES}
    c = ctypes
    assert sig["hb_merkle_encode_many"][1:] == (c.c_int, [c.c_void_p, c.POINTER(_native.MerkleEncodeDesc),
                                                          c.c_uint64, c.c_uint32])
    assert sig["hb_merkle_leaves_many"][1:] == (c.c_int, [c.c_void_p, c.POINTER(_native.MerkleLeafDesc),
                                                          c.c_uint64, c.c_uint32])
    # the descriptors are 8-byte words in the header's order
    assert [f[0] for f in _native.MerkleEncodeDesc._fields_] == [
        "key", "key_len", "seed", "seed_len", "n", "filesz", "chunksz", "data", "len", "nodes_out", "leaves_out",
        "offsets_out"]
    assert ctypes.sizeof(_native.MerkleEncodeDesc) == 12 * 8
    assert [f[0] for f in _native.MerkleLeafDesc._fields_] == [
        "seed", "seed_len", "filesz", "chunksz", "data", "len", "leaf_out", "offset_out"]
    assert ctypes.sizeof(_native.MerkleLeafDesc) == 8 * 8
    with open(os.path.join(ROOT, "include", "hbswizzle.h")) as fh:
        header = " ".join(fh.read().split())
    assert ("int hb_merkle_encode_many(hb_ctx *ctx, const hb_merkle_encode_desc *files, uint64_t nfiles, "
            "uint32_t flags);") in header
    assert ("int hb_merkle_leaves_many(hb_ctx *ctx, const hb_merkle_leaf_desc *proofs, uint64_t nproofs, "
            "uint32_t flags);") in header
    assert "#define HB_MERKLE_CHAIN_HOST %du" % _native.HB_MERKLE_CHAIN_HOST in header
    assert "#define HB_MERKLE_CHAIN_DEVICE %du" % _native.HB_MERKLE_CHAIN_DEVICE in header
    assert "#define HB_MERKLE_MAX_N %du" % _native.HB_MERKLE_MAX_N in header


def test_alias_package_is_unchanged():
    import heartbeat
    import heartbeat.Merkle
    import heartbeat_amd.Merkle
    assert heartbeat.Merkle.MerkleHelper is heartbeat_amd.Merkle.MerkleHelper
    for name in ("Merkle", "MerkleTree", "Challenge", "Tag", "State", "Proof"):
        with pytest.raises(AttributeError, match="outside this build's scope"):
            getattr(heartbeat.Merkle, name)
