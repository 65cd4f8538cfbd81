// hb_merkle.hpp -- per-lane arithmetic of the Merkle scheme
// (heartbeat/Merkle/Merkle.py, MerkleTree.py): the seed chain's HMAC link on
// cached key midstates, the leaf hash, the node hash with the reference's
// empty-child rule, the tree order and one tree node from its children.
//
// Every function is HB_HHD: inlined into the kernels of hb_kern_merkle.hip,
// called by the host runtime (the host chain, the keys' midstates and the
// first link, hb_merkle_host.hpp) and compiled as plain C++ by
// tests/merkle_emul.  Digests are 8 big-endian words; a node or seed buffer
// in memory holds the digests' bytes, so a u32 load of it is byte-swapped.
#pragma once
#include "hb_lane.hpp"

// most leaves of one tree on the GPU path (order <= 16)
#define HB_MERKLE_MAX_LEAVES 65536u

// SHA-256 compression in portable C++: what the host pass of a HIP unit calls,
// where the lane functions of hb_lane.hpp (device-only there) cannot be.
HB_HHD void hb_mk_compress_portable(u32 st[8], u32 W[16]) {
    const u32 K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u,
        0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,
        0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu,
        0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u,
        0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
        0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
        0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u,
        0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u,
        0xc67178f2u};
    auto rr = [](u32 x, u32 n) { return (x >> n) | (x << (32u - n)); };
    u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int t = 0; t < 64; ++t) {
        u32 w;
        if (t < 16) {
            w = W[t];
        } else {
            const u32 w15 = W[(t - 15) & 15], w2 = W[(t - 2) & 15];
            w = W[t & 15] + (rr(w15, 7) ^ rr(w15, 18) ^ (w15 >> 3)) + W[(t - 7) & 15] +
                (rr(w2, 17) ^ rr(w2, 19) ^ (w2 >> 10));
            W[t & 15] = w;
        }
        const u32 t1 = h + (rr(e, 6) ^ rr(e, 11) ^ rr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w;
        const u32 t2 = (rr(a, 2) ^ rr(a, 13) ^ rr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// One compression (W clobbered): the lane's hb_sha256_compress in a kernel and
// in a plain C++ build, the portable one in the host pass of a HIP unit.
HB_HHD void hb_mk_compress(u32 st[8], u32 W[16]) {
#if defined(__HIP__) && !defined(__HIP_DEVICE_COMPILE__)
    hb_mk_compress_portable(st, W);
#else
    hb_sha256_compress(st, W);
#endif
}

HB_HHD void hb_mk_init(u32 st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

HB_HHD u32 hb_mk_bswap(u32 x) {
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

// Finish a SHA-256 whose first `done` bytes (a multiple of 64) are in st: the
// n bytes at m, then the padding for a message of done + n bytes.
HB_HHD void hb_mk_sha256_tail(u32 st[8], u64 done, const unsigned char *m, u64 n) {
    const u64 nblk = (n + 9 + 63) / 64;
    const u64 bits = (done + n) * 8;
    for (u64 b = 0; b < nblk; ++b) {
        u32 W[16];
        for (int t = 0; t < 16; ++t) {
            u32 w = 0;
            for (int k = 0; k < 4; ++k) {
                const u64 p = 64 * b + 4 * (u64)t + (u64)k;
                w = (w << 8) | (p < n ? (u32)m[p] : (p == n ? 0x80u : 0u));
            }
            W[t] = w;
        }
        if (b == nblk - 1) {
            W[14] |= (u32)(bits >> 32);
            W[15] |= (u32)bits;
        }
        hb_mk_compress(st, W);
    }
}

// The ipad and opad midstates of an HMAC-SHA256 key of any length (RFC 2104:
// a key longer than the 64-byte block is hashed first; key_len = 0 is the
// all-zero block, Merkle.get_public's b'').  Once per file: a chain link is
// then two compressions.
struct HbMkKey {
    u32 ipad[8], opad[8];
};

HB_HHD void hb_mk_key(const unsigned char *key, u64 key_len, HbMkKey &K) {
    u32 kw[16];
    for (int t = 0; t < 16; ++t) kw[t] = 0;
    if (key_len > 64) {
        u32 h[8];
        hb_mk_init(h);
        hb_mk_sha256_tail(h, 0, key, key_len);
        for (int t = 0; t < 8; ++t) kw[t] = h[t];
    } else {
        for (u64 k = 0; k < key_len; ++k) kw[k >> 2] |= (u32)key[k] << (24 - 8 * (k & 3));
    }
    u32 W[16];
    for (int t = 0; t < 16; ++t) W[t] = kw[t] ^ 0x36363636u;
    hb_mk_init(K.ipad);
    hb_mk_compress(K.ipad, W);
    for (int t = 0; t < 16; ++t) W[t] = kw[t] ^ 0x5c5c5c5cu;
    hb_mk_init(K.opad);
    hb_mk_compress(K.opad, W);
}

// The outer hash of an HMAC: SHA-256(opad block || inner digest).
HB_HHD void hb_mk_outer(const HbMkKey &K, const u32 inner[8], u32 out[8]) {
    u32 W[16];
    for (int t = 0; t < 8; ++t) W[t] = inner[t];
    W[8] = 0x80000000u;
    for (int t = 9; t < 15; ++t) W[t] = 0;
    W[15] = (64 + 32) * 8;
    for (int t = 0; t < 8; ++t) out[t] = K.opad[t];
    hb_mk_compress(out, W);
}

// HMAC-SHA256(key, m) of any message: the chain's first link, from the
// caller's seed of any length (Merkle.py:357).
HB_HHD void hb_mk_hmac(const HbMkKey &K, const unsigned char *m, u64 n, u32 out[8]) {
    u32 inner[8];
    for (int t = 0; t < 8; ++t) inner[t] = K.ipad[t];
    hb_mk_sha256_tail(inner, 64, m, n);
    hb_mk_outer(K, inner, out);
}

// One chain link s' = HMAC-SHA256(key, s) of a 32-byte seed s
// (MerkleHelper.get_next_seed, Merkle.py:451-460): two compressions.
HB_HHD void hb_mk_link(const HbMkKey &K, const u32 s[8], u32 out[8]) {
    u32 W[16], inner[8];
    for (int t = 0; t < 8; ++t) W[t] = s[t];
    W[8] = 0x80000000u;
    for (int t = 9; t < 15; ++t) W[t] = 0;
    W[15] = (64 + 32) * 8;
    for (int t = 0; t < 8; ++t) inner[t] = K.ipad[t];
    hb_mk_compress(inner, W);
    hb_mk_outer(K, inner, out);
}

// The leaf hash SHA-256(blob || ascii-decimal(index)) (MerkleLeaf.get_hash,
// MerkleTree.py:50-53): 32 bytes and at most 10 digits, one compression.
HB_HHD void hb_mk_leaf_hash(const u32 blob[8], u32 index, u32 out[8]) {
    u32 W[16];
    for (int t = 0; t < 8; ++t) W[t] = blob[t];
    for (int t = 8; t < 16; ++t) W[t] = 0;
    u32 nd = 1;
    for (u32 v = index; v >= 10; v /= 10) ++nd;
    u32 v = index;
    for (u32 k = nd; k-- > 0;) {   // least significant digit last
        const u32 pos = 32 + k;
        W[pos >> 2] |= (0x30u + v % 10) << (24 - 8 * (pos & 3));
        v /= 10;
    }
    const u32 end = 32 + nd;
    W[end >> 2] |= 0x80u << (24 - 8 * (end & 3));
    W[15] = end * 8;
    hb_mk_init(out);
    hb_mk_compress(out, W);
}

// The hash of an interior node from its children (MerkleTree.py:162-173): a
// child that is empty contributes nothing.  nchild = 2: SHA-256(l || r), two
// compressions; 1: SHA-256(l), the parent of one leaf hash and one empty slot;
// 0: SHA-256(b""), the parent of two empty slots (32 non-empty bytes itself).
HB_HHD void hb_mk_node_hash(const u32 l[8], const u32 r[8], u32 nchild, u32 out[8]) {
    u32 W[16];
    hb_mk_init(out);
    if (nchild == 2) {
        for (int t = 0; t < 8; ++t) {
            W[t] = l[t];
            W[8 + t] = r[t];
        }
        hb_mk_compress(out, W);
        W[0] = 0x80000000u;
        for (int t = 1; t < 15; ++t) W[t] = 0;
        W[15] = 64 * 8;
    } else if (nchild == 1) {
        for (int t = 0; t < 8; ++t) W[t] = l[t];
        W[8] = 0x80000000u;
        for (int t = 9; t < 15; ++t) W[t] = 0;
        W[15] = 32 * 8;
    } else {
        W[0] = 0x80000000u;
        for (int t = 1; t < 16; ++t) W[t] = 0;
    }
    hb_mk_compress(out, W);
}

// The order of a tree of n >= 1 leaves: 0 for one leaf, else the bit length
// of n - 1 -- the reference's int(ceil(log(n, 2))) (MerkleTree.py:246-252)
// wherever the float expression is exact (every n < 2^17 at the least).
HB_HHD u32 hb_mk_order(u64 n) {
    u32 o = 0;
    for (u64 v = n > 0 ? n - 1 : 0; v; v >>= 1) ++o;
    return o;
}

// Node j of level i (1 = the leaves' parents .. order = the root) of a tree
// of n leaves: node p + j - 1, p = 2^(order - i) (MerkleTree.py:162-173), from
// its children 2k + 1 and 2k + 2.  nodes: the tree's (2 << order) x 32 bytes.
// The leaves' parents count their children by position -- leaf slots >= n and
// the unused last entry are empty -- every level above has two 32-byte ones.
HB_HHD void hb_mk_tree_node(u32 *nodes, u32 order, u32 n, u32 i, u32 j) {
    const u32 p = 1u << (order - i);
    const u32 k = p + j - 1;
    u32 nchild = 2;
    if (i == 1) nchild = 2 * j + 1 < n ? 2u : (2 * j < n ? 1u : 0u);
    u32 l[8], r[8], h[8];
    const u32 *cl = nodes + (size_t)(2 * k + 1) * 8;
    for (int t = 0; t < 8; ++t) {
        l[t] = nchild >= 1 ? hb_mk_bswap(cl[t]) : 0u;
        r[t] = nchild >= 2 ? hb_mk_bswap(cl[8 + t]) : 0u;
    }
    hb_mk_node_hash(l, r, nchild, h);
    for (int t = 0; t < 8; ++t) nodes[(size_t)k * 8 + t] = hb_mk_bswap(h[t]);
}
