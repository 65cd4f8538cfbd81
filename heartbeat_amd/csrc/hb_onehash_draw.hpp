// hb_onehash_draw.hpp -- the positions of OneHash.pick_blocks
// (heartbeat/OneHash/OneHash.py:170-189): Python's module-level generator
// seeded with the root seed, then randint(0, file_size - 1) for every
// challenge.  Bit-exact with CPython's `random` (seed version 2): MT19937
// seeded by init_by_array over a key the host makes from the root seed (for
// str / bytes the seed followed by its SHA-512, read as one big-endian
// integer; for an int its absolute value; 32-bit words, least significant
// first), and _randbelow(len) by rejection: with k = bit_length(len), draw
// getrandbits(k) until it is below len.
//
// Every function is HB_HHD: inlined into hb_onehash_draw_kernel
// (hb_kern_onehash.hip), where a wave shares one state in LDS, and compiled
// as plain C++ by tests/onehash_draw_emul, which walks the same steps one
// lane at a time (hb_mt_draw_serial).
#pragma once
#include "hb_lane.hpp"

#define HB_MT_N 624u
#define HB_MT_M 397u
#define HB_MT_STATE_WORDS 625u   // mt[0..623], then the index: what random.getstate() holds
#define HB_MT_CHUNK 64u          // elements regenerated, and attempts tested, side by side

// ------------------------------------------------------------------ seeding
// init_genrand(19650218), then init_by_array(key): max(624, nkey) steps that
// add key[j] + j, then 623 that subtract i, then mt[0] = 0x80000000.  A serial
// recurrence: every step reads the element before it, carried in `prev`, so
// that the only memory reads on the chain are of elements written long before.
HB_HHD void hb_mt_seed(u32 *mt, const u32 *key, u64 nkey) {
    u32 prev = 19650218u;
    mt[0] = prev;
    HB_NOUNROLL
    for (u32 i = 1; i < HB_MT_N; ++i) {
        prev = 1812433253u * (prev ^ (prev >> 30)) + i;
        mt[i] = prev;
    }
    u32 i = 1;
    u64 j = 0;
    prev = mt[0];
    const u64 steps = nkey > HB_MT_N ? nkey : HB_MT_N;
    HB_NOUNROLL
    for (u64 s = 0; s < steps; ++s) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + key[j] + (u32)j;
        mt[i] = prev;
        if (++i >= HB_MT_N) {
            mt[0] = prev;
            i = 1;
        }
        if (++j >= nkey) j = 0;
    }
    HB_NOUNROLL
    for (u32 s = 0; s < HB_MT_N - 1; ++s) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - i;
        mt[i] = prev;
        if (++i >= HB_MT_N) {
            mt[0] = prev;
            i = 1;
        }
    }
    mt[0] = 0x80000000u;
}

// ------------------------------------------------------------------ regeneration
// Element i of the next array.  It reads mt[i] and mt[i + 1] of the old array
// and mt[i + 397]: old for i < 227, the new mt[i - 227] for 227 <= i < 623;
// i = 623 reads the new mt[0] (as its neighbour) and the new mt[396].  So
// elements are made in index order, HB_MT_CHUNK at a time: a chunk reads
// before it writes (its neighbours mt[i + 1] are its own elements), and every
// new element it reads lies 227 or more behind it, in a chunk already written.
HB_HHD u32 hb_mt_next(const u32 *mt, u32 i) {
    const u32 nb = mt[i + 1 < HB_MT_N ? i + 1 : 0];
    const u32 far = mt[i + HB_MT_M < HB_MT_N ? i + HB_MT_M : i + HB_MT_M - HB_MT_N];
    const u32 y = (mt[i] & 0x80000000u) | (nb & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

HB_HHD u32 hb_mt_temper(u32 y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// ------------------------------------------------------------------ the draw
// bit_length(len), 1..64 for len >= 1.
HB_HHD u32 hb_mt_bits(u64 len) {
    u32 k = 0;
    while (len) {
        ++k;
        len >>= 1;
    }
    return k;
}

// Words of the stream one attempt consumes, accepted or not: getrandbits(k)
// is one word for k <= 32, two above.  624 is even: a pair never straddles a
// regeneration.
HB_HHD u32 hb_mt_words(u32 k) { return k > 32u ? 2u : 1u; }

// Attempt `a` of an array (its words mt[a * w .. a * w + w)): getrandbits(k)
// -- the tempered word >> (32 - k), or the first word as the low 32 bits and
// the second >> (64 - k) above them -- into r; accepted when r < len.
HB_HHD bool hb_mt_attempt(const u32 *mt, u32 a, u64 len, u32 k, u64 &r) {
    if (k <= 32u) {
        r = hb_mt_temper(mt[a]) >> (32u - k);
    } else {
        const u64 lo = hb_mt_temper(mt[2u * a]);
        const u64 hi = hb_mt_temper(mt[2u * a + 1u]) >> (64u - k);
        r = (hi << 32) | lo;
    }
    return r < len;
}

// num positions in [0, len) (len >= 1 when num > 0) from a seeded state, one
// lane at a time in the kernel's order; returns the index random.getstate()
// ends on.  The twist is lazy: an array is regenerated only when an attempt
// needs a word and none is left, so after exactly 624 * m words the state is
// the m-th array with index 624.
HB_HHD u32 hb_mt_draw_serial(u32 *mt, u64 len, u64 num, u64 *out) {
    const u32 k = hb_mt_bits(len), w = hb_mt_words(k);
    const u32 attempts = HB_MT_N / w;
    u32 used = HB_MT_N;
    u64 made = 0;
    while (made < num) {
        for (u32 base = 0; base < HB_MT_N; base += HB_MT_CHUNK) {
            u32 v[HB_MT_CHUNK];
            for (u32 l = 0; l < HB_MT_CHUNK && base + l < HB_MT_N; ++l) v[l] = hb_mt_next(mt, base + l);
            for (u32 l = 0; l < HB_MT_CHUNK && base + l < HB_MT_N; ++l) mt[base + l] = v[l];
        }
        for (u32 a = 0; a < attempts && made < num; ++a) {
            u64 r;
            if (hb_mt_attempt(mt, a, len, k, r)) out[made++] = r;
            used = (a + 1) * w;
        }
    }
    return used;
}
