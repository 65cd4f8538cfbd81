"""The Merkle heartbeat (heartbeat/Merkle): the scheme's classes, the helper
and the tree, with the reference package's names; GPU encode, prove and
batches (Merkle.py), the host tree (MerkleTree.py)."""
from .Merkle import Challenge, Tag, State, Proof, Merkle, MerkleHelper   # NOQA
from .Merkle import DEFAULT_BUFFER_SIZE, DEFAULT_CHUNK_SIZE, DeviceFile  # NOQA
from .MerkleTree import MerkleTree  # NOQA
