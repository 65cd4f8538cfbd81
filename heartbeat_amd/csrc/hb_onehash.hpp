// hb_onehash.hpp -- per-lane arithmetic of the OneHash scheme
// (heartbeat/OneHash/OneHash.py): which bytes of the file a challenge covers
// (the plan rule, with the reference's short read at a wrap), the SHA-256 of
// those bytes and the seed, and one link of the seed chain on a secret
// prepared once per file.
//
// Every function is HB_HHD: inlined into the kernels of hb_kern_onehash.hip,
// called by the host runtime (hb_onehash_host.hpp) and compiled as plain C++
// by tests/onehash_emul.  Digests are 8 big-endian words.
#pragma once
#include "hb_merkle.hpp"

#define HB_ONEHASH_CHUNK 1024u      // most file bytes of one response (OneHash.py:120)
#define HB_ONEHASH_MAX_SEED 64u     // longest seed of a response on the GPU path
#define HB_ONEHASH_MAX_SECRET 87u   // longest secret of a chain on the GPU path: two compressions a link

// The file bytes of one response: data[off0 : off0 + len0] || data[off1 : off1 + len1].
struct HbOhPlan {
    u64 off0, len0, off1, len1;
};

// The chunk length of a file (OneHash.py:120).
HB_HHD u64 hb_oh_chunk(u64 file_size) {
    const u64 tenth = file_size / 10;
    return tenth < HB_ONEHASH_CHUNK ? tenth : HB_ONEHASH_CHUNK;
}

// The plan rule (OneHash.py:120-134) for 0 <= block < file_size, or block = 0
// of an empty file.  Without a wrap the c bytes at block.  With one,
// a = block - (file_size - c) > 0: the reference reads a bytes at block -- only
// file_size - block = c - a are left there -- and then c - a bytes from 0, so
// the file part is min(a, c - a) + (c - a) bytes, fewer than c when a > c / 2.
HB_HHD HbOhPlan hb_oh_plan(u64 file_size, u64 block) {
    const u64 c = hb_oh_chunk(file_size);
    HbOhPlan P;
    P.off0 = block;
    P.off1 = 0;
    if (block <= file_size - c) {
        P.len0 = c;
        P.len1 = 0;
    } else {
        const u64 a = block - (file_size - c);
        P.len0 = a < c - a ? a : c - a;
        P.len1 = c - a;
    }
    return P;
}

// Both segments inside [0, len)?  What a lane asks before it reads.
HB_HHD bool hb_oh_plan_inside(const HbOhPlan &P, u64 len) {
    return P.off0 <= len && len - P.off0 >= P.len0 && P.off1 <= len && len - P.off1 >= P.len1;
}

// SHA-256(data[off0 : +len0] || data[off1 : +len1] || seed[0 : seed_len]):
// segments of any alignment and length.  A block that lies whole inside one
// file segment is read as 17 aligned dwords, funnel-shifted -- where all 17
// stay inside [data, data + len); a block that straddles a segment's end, the
// seed and the padding are put together bytewise.  The caller has checked the
// segments against len (hb_oh_plan_inside).
HB_HHD void hb_oh_hash(const unsigned char *data, u64 len, const HbOhPlan &P, const unsigned char *seed,
                       u64 seed_len, u32 out[8]) {
    const u64 l0 = P.len0, l01 = P.len0 + P.len1;
    const u64 n = l01 + seed_len;
    const u64 nblk = (n + 9 + 63) / 64;
    const u64 bits = n * 8;
    const uintptr_t lo = (uintptr_t)data, hi = (uintptr_t)data + len;
    u32 st[8], W[16];
    hb_mk_init(st);
    HB_NOUNROLL
    for (u64 b = 0; b < nblk; ++b) {
        const u64 p0 = 64 * b;
        // the block's first byte in the file, if one segment holds all of it
        bool whole = false;
        u64 at = 0;
        if (p0 + 64 <= l0) {
            whole = true;
            at = P.off0 + p0;
        } else if (p0 >= l0 && p0 + 64 <= l01) {
            whole = true;
            at = P.off1 + (p0 - l0);
        }
        const uintptr_t a = ((uintptr_t)data + at) & ~(uintptr_t)3;
        if (whole && a >= lo && a + 68 <= hi) {
            const u32 sh = 8u * (u32)(((uintptr_t)data + at) & 3u);
            const u32 *q = (const u32 *)a;
            u32 prev = q[0];
            HB_UNROLL
            for (int t = 0; t < 16; ++t) {
                const u32 nx = q[t + 1];
                W[t] = hb_mk_bswap(sh ? (prev >> sh) | (nx << (32u - sh)) : prev);
                prev = nx;
            }
        } else {
            HB_UNROLL
            for (int t = 0; t < 16; ++t) {
                u32 w = 0;
                for (int k = 0; k < 4; ++k) {
                    const u64 p = p0 + 4 * (u64)t + (u64)k;
                    u32 byte;
                    if (p < l0) byte = data[P.off0 + p];
                    else if (p < l01) byte = data[P.off1 + (p - l0)];
                    else if (p < n) byte = seed[p - l01];
                    else byte = p == n ? 0x80u : 0u;
                    w = (w << 8) | byte;
                }
                W[t] = w;
            }
            if (b == nblk - 1) {
                W[14] |= (u32)(bits >> 32);
                W[15] |= (u32)bits;
            }
        }
        hb_mk_compress(st, W);
    }
    for (int t = 0; t < 8; ++t) out[t] = st[t];
}

// A chain's secret, prepared once per file: the message words of
// SHA-256(s || secret) after the 32 bytes of s, padding and length included.
// nblk = 1 for secrets of up to 23 bytes, 2 up to 87.
struct HbOhSecret {
    u32 w[24];   // words 8..15 of the first block, then the second block
    u32 nblk;
};

// False (S untouched) for a secret too long for two compressions.
HB_HHD bool hb_oh_secret(const unsigned char *secret, u64 secret_len, HbOhSecret &S) {
    if (secret_len > HB_ONEHASH_MAX_SECRET) return false;
    for (int t = 0; t < 24; ++t) S.w[t] = 0;
    for (u64 k = 0; k < secret_len; ++k) S.w[k >> 2] |= (u32)secret[k] << (24 - 8 * (k & 3));
    S.w[secret_len >> 2] |= 0x80u << (24 - 8 * (secret_len & 3));
    S.nblk = secret_len <= 23 ? 1u : 2u;
    S.w[S.nblk == 1 ? 7 : 23] = (u32)(32 + secret_len) * 8;
    return true;
}

// One chain link s' = SHA-256(s || secret) (OneHash.py:162-166).
HB_HHD void hb_oh_link(const HbOhSecret &S, const u32 s[8], u32 out[8]) {
    u32 W[16];
    for (int t = 0; t < 8; ++t) {
        W[t] = s[t];
        W[8 + t] = S.w[t];
    }
    hb_mk_init(out);
    hb_mk_compress(out, W);
    if (S.nblk == 2) {
        for (int t = 0; t < 16; ++t) W[t] = S.w[8 + t];
        hb_mk_compress(out, W);
    }
}
