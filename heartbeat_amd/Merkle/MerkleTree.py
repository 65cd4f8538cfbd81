"""The Merkle scheme's tree (heartbeat/Merkle/MerkleTree.py) on the host.

Numbering, as the reference's: node 0 is the root, the children of node k are
2k + 1 and 2k + 2, and the 2^order leaf slots are nodes 2^order - 1 onwards;
``nodes`` has 2 * 2^order entries, the last one unused::

    nodes                     0
                  1                       2
              3       4               5       6
    leaves    0   1   2   3           4   -   -   -      (n = 5, order 3)

A leaf's node is SHA-256(blob || str(index)).  An interior node hashes its
children, and a child that is empty (b'') contributes nothing: the parent of
one leaf hash and one empty slot is SHA-256 of 32 bytes, the parent of two
empty slots is SHA-256(b'') -- 32 non-empty bytes, so every level above hashes
64 bytes.  Empty slots are the leaf slots j >= n and the unused last entry.

This is a ``hashlib`` implementation: ``Merkle.verify`` runs it (order + 1
small hashes), and it is what the GPU tree (hb_merkle_tree_kernel) is tested
against.  A tree that came from the GPU keeps the raw node buffer and
materialises ``nodes`` (a list of bytes) on first use: a batch of 256 files
would otherwise build 131,072 small objects that a prove never looks at.

``get_order(n)`` is 0 for n = 1 and the bit length of n - 1 above; the
reference's ``int(ceil(log(n, 2)))`` equals it for every n < 2^17 and first
goes wrong, being a float expression, at 2^29.
"""
import hashlib

from ..util import hb_encode, hb_decode


class MerkleLeaf(object):
    """A leaf: its index and payload (the chunk's HMAC)."""

    def __init__(self, index, blob):
        self.index = index
        self.blob = blob

    def __eq__(self, other):
        return isinstance(other, MerkleLeaf) and self.index == other.index and self.blob == other.blob

    def get_hash(self):
        return hashlib.sha256(self.blob + str(self.index).encode()).digest()

    def todict(self):
        return {'index': self.index, 'blob': hb_encode(self.blob)}

    @staticmethod
    def fromdict(dict):
        return MerkleLeaf(dict['index'], hb_decode(dict['blob']))


class MerkleBranch(object):
    """The pairs of nodes between a leaf and the root, leaf level first."""

    def __init__(self, order):
        self.rows = [(b'', b'')] * order

    def __eq__(self, other):
        return isinstance(other, MerkleBranch) and self.rows == other.rows

    def get_left(self, i):
        return self.rows[i][0]

    def get_right(self, i):
        return self.rows[i][1]

    def set_row(self, i, value):
        self.rows[i] = value

    def get_order(self):
        return len(self.rows)

    def todict(self):
        return {'rows': [(hb_encode(l), hb_encode(r)) for l, r in self.rows]}

    @staticmethod
    def fromdict(dict):
        self = MerkleBranch(len(dict['rows']))
        self.rows = [(hb_decode(x[0]), hb_decode(x[1])) for x in dict['rows']]
        return self


def _pair_hash(left, right):
    # an empty child adds nothing to the hash
    return hashlib.sha256(left + right).digest()


class MerkleTree(object):
    """A static tree: ``add_leaf()`` the payloads, then ``build()``."""

    def __init__(self):
        self._nodes = list()
        self._raw = None      # a GPU tree's node buffer: (bytes, n) until `nodes` is used
        self.order = 0
        self.leaves = list()

    @classmethod
    def _from_raw(cls, raw, order, n):
        """The stripped tree of a GPU encode: `raw` is (2 << order) * 32 bytes,
        empty slots zero (hb_merkle_encode_many's nodes_out)."""
        self = cls()
        self._raw = (bytes(raw), int(n))
        self.order = int(order)
        return self

    def _is_empty(self, k, n):
        first = (1 << self.order) - 1
        return k >= first + n

    def _node(self, k):
        if self._raw is None:
            return self._nodes[k]
        raw, n = self._raw
        return b'' if self._is_empty(k, n) else raw[32 * k:32 * k + 32]

    @property
    def nodes(self):
        if self._raw is not None:
            raw, n = self._raw
            self._nodes = [b'' if self._is_empty(k, n) else raw[32 * k:32 * k + 32]
                           for k in range(2 << self.order)]
            self._raw = None
        return self._nodes

    @nodes.setter
    def nodes(self, value):
        self._raw = None
        self._nodes = value

    def __eq__(self, other):
        return (isinstance(other, MerkleTree) and self.nodes == other.nodes and
                self.order == other.order and self.leaves == other.leaves)

    def todict(self):
        return {'nodes': hb_encode(self.nodes),
                'order': self.order,
                'leaves': [x.todict() for x in self.leaves]}

    @staticmethod
    def fromdict(dict):
        self = MerkleTree()
        self.nodes = hb_decode(dict['nodes'])
        self.order = dict['order']
        self.leaves = [MerkleLeaf.fromdict(x) for x in dict['leaves']]
        return self

    def add_leaf(self, leaf_blob):
        """Append a leaf payload; ``build()`` makes the tree."""
        self.leaves.append(MerkleLeaf(len(self.leaves), leaf_blob))

    def build(self):
        """The nodes from the leaves that were added, level by level."""
        self.order = MerkleTree.get_order(len(self.leaves))
        width = 1 << self.order
        nodes = [b''] * (2 * width)
        for j, leaf in enumerate(self.leaves):
            nodes[width - 1 + j] = leaf.get_hash()
        for level in range(self.order - 1, -1, -1):
            first = (1 << level) - 1
            for k in range(first, 2 * first + 1):
                nodes[k] = _pair_hash(nodes[2 * k + 1], nodes[2 * k + 2])
        self.nodes = nodes

    def get_branch(self, i):
        """The branch of leaf i: per level the pair of nodes that holds the
        path's node, from the leaf level up to the root's children."""
        branch = MerkleBranch(self.order)
        j = i + (1 << self.order) - 1
        for k in range(self.order):
            left = j if MerkleTree.is_left(j) else j - 1
            branch.set_row(k, (self._node(left), self._node(left + 1)))
            j = MerkleTree.get_parent(j)
        return branch

    def get_root(self):
        return self._node(0)

    def strip_leaves(self):
        """Drop the leaf payloads (the tag keeps only the nodes)."""
        self.leaves = list()

    @staticmethod
    def get_parent(i):
        return (i + 1) // 2 - 1

    @staticmethod
    def get_partner(i):
        return i + 1 if MerkleTree.is_left(i) else i - 1

    @staticmethod
    def is_left(i):
        return i % 2 != 0

    @staticmethod
    def get_left_child(i):
        return 2 * i + 1

    @staticmethod
    def get_right_child(i):
        return 2 * i + 2

    @staticmethod
    def get_order(n):
        """Levels below the root of a tree of n leaves: 0 for one leaf, else
        the bit length of n - 1.  n < 1 has no tree (the reference fails
        inside math.log)."""
        n = int(n)
        if n < 1:
            raise ValueError("a tree needs at least one leaf")
        return (n - 1).bit_length()

    @staticmethod
    def verify_branch(leaf, branch, root):
        """True if `branch` leads from `leaf` to `root`: the running hash must
        be one of the pair at every level, and the last one the root."""
        try:
            lh = leaf.get_hash()
        except Exception:
            return False
        for i in range(branch.get_order()):
            left, right = branch.get_left(i), branch.get_right(i)
            if left != lh and right != lh:
                return False
            lh = _pair_hash(left, right)
        return root == lh
