// Walks the pure host header of the mixed-owner batches
// (heartbeat_amd/csrc/hb_mixed_host.hpp) over randomised mixes of primes,
// sector counts, key lengths and challenge lengths: the class partition, the
// grouping of each class (hb_batch_groups with the mixed costs), every
// group's arena against the items' costs, the ragged column / alpha-slot
// prefix sums, the two workgroup tables, and the distinct-prime cache.  Built
// with -fsanitize=address,undefined and run by tests/test_mixed_host.py.
// Exit status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hb_mixed_host.hpp"

static int g_checks = 0, g_bad = 0;

static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    ++g_checks;
    if (!ok) {
        ++g_bad;
        if (g_bad < 50) printf("FAIL %s (%lld, %lld)\n", what, a, b);
    }
}

static uint64_t g_x = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    g_x = g_x * 6364136223846793005ull + 1442695040888963407ull;
    return g_x >> 17;
}

struct Item {
    int bits;
    uint32_t nl, nr, S, chunks;
    uint64_t up_files;
};

static Item some_item() {
    static const int bits[] = {20, 61, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025, 2048};
    static const uint32_t chunks[] = {0, 1, 15, 16, 17, 33, 255, 256, 257, 511, 512, 513, 1000};
    static const uint32_t S[] = {1, 3, 10, 16, 40};
    static const uint64_t keys[] = {16, 24, 32};
    Item I;
    I.bits = bits[rnd() % 12];
    I.nl = hb_mx_limbs(I.bits);
    I.nr = hb_mx_rounds(keys[rnd() % 3]);
    I.S = S[rnd() % 5];
    I.chunks = chunks[rnd() % 13];
    I.up_files = rnd() % 3 ? hb_up16(rnd() % 5000) + hb_up16(rnd() % 900) : 0;
    return I;
}

// sizes as the runtime's batch_sizes<NL>() has them, to the rounding
static HbBatchSizes sizes_of(uint32_t nl) {
    HbBatchSizes z = {};
    z.prf2 = 60 * 4 + 2 * 4 + 24;
    z.prf = 60 * 4 + nl * 4 + 24;
    z.limbs = nl * 4;
    z.vproof = 16;
    z.pproof = 48;
    return z;
}
static uint64_t rec_of(uint32_t nl) { return 2 * 4 * (uint64_t)nl + 16 + 32; }

static void check_arena(const char *what, const HbArena &L, const std::vector<uint64_t> &sizes, uint32_t n_up, uint64_t cost) {
    expect(L.n == sizes.size(), what, (long long)L.n, (long long)sizes.size());
    if (L.n != sizes.size()) return;
    uint64_t end = 0, sum = 0;
    for (uint32_t s = 0; s < L.n; ++s) {
        expect(L.off[s] % 16 == 0, "offset is a multiple of 16", s);
        expect(L.off[s] >= end && L.off[s] < end + 16, "sections in order, no overlap, no gap of 16", s);
        end = L.off[s] + sizes[s];
        sum += sizes[s];
        if (s + 1 == n_up) expect(L.up_bytes == end, "up_bytes ends the last uploaded section", s);
    }
    expect(L.total == end, "total ends the last section");
    expect(sum == cost, "the sections are exactly what the items cost", (long long)sum, (long long)cost);
    expect(L.total <= cost + 16 * (uint64_t)L.n, "total <= costs + 16 x sections", (long long)L.total, (long long)cost);
}

static void walk_mix(uint64_t n, uint64_t cap_units, uint64_t cap_bytes) {
    std::vector<Item> items;
    std::vector<uint32_t> nl, nr;
    for (uint64_t i = 0; i < n; ++i) {
        items.push_back(some_item());
        nl.push_back(items.back().nl);
        nr.push_back(items.back().nr);
    }
    // ---- the partition: every item in exactly one class, input order inside a class
    const std::vector<HbMxClass> classes = hb_mixed_partition(nl.data(), nr.data(), n);
    std::vector<int> seen((size_t)n, 0);
    for (size_t k = 0; k < classes.size(); ++k) {
        const HbMxClass &K = classes[k];
        expect(!K.items.empty(), "no empty class");
        for (size_t j = 0; j < k; ++j) expect(classes[j].nl != K.nl || classes[j].nr != K.nr, "one class per (limbs, rounds)");
        if (k) expect(classes[k - 1].items[0] < K.items[0], "classes in the order of their first item");
        for (size_t a = 0; a < K.items.size(); ++a) {
            const uint64_t i = K.items[a];
            expect(i < n, "an item of the call");
            if (i >= n) continue;
            ++seen[(size_t)i];
            expect(items[(size_t)i].nl == K.nl && items[(size_t)i].nr == K.nr, "the item's own class");
            if (a) expect(K.items[a - 1] < i, "input order inside a class");
        }
    }
    for (uint64_t i = 0; i < n; ++i) expect(seen[(size_t)i] == 1, "every item in exactly one class", (long long)i, seen[(size_t)i]);

    // ---- each class planned as the runtime plans it, prove and verify
    for (const HbMxClass &K : classes) {
        const HbBatchSizes z = sizes_of(K.nl);
        const uint64_t rec = rec_of(K.nl);
        for (int verify = 0; verify < 2; ++verify) {
            std::vector<HbCbItemReq> req;
            std::vector<uint64_t> cand;
            for (uint64_t i : K.items) {
                const Item &I = items[(size_t)i];
                if (!verify && I.chunks == 0) continue;   // the prove: zero sums, no descriptor in a group
                HbCbItemReq R = {};
                const uint64_t nj = verify ? (I.S + 15) / 16 + 2 * ((I.chunks + 15) / 16) : 2 * ((I.chunks + 15) / 16);
                R.units = I.chunks;
                R.bytes = verify ? hb_mverify_cost(z, rec, nj, I.chunks, I.S) : hb_mprove_cost(z, rec, nj, I.chunks, I.S, I.up_files);
                cand.push_back(i);
                req.push_back(R);
            }
            const HbCbPlan plan = hb_batch_groups(req.data(), req.size(), cap_units, cap_units, cap_bytes);
            uint64_t placed = plan.through.size();
            for (const HbCbGroup &G : plan.groups) {
                placed += G.nitems;
                const uint64_t np = G.nitems;
                std::vector<uint32_t> S, chunks;
                uint64_t cost = 0, nj = 0, up = 0, terms = 0;
                for (uint64_t f = 0; f < np; ++f) {
                    const uint64_t at = plan.order[(size_t)(G.item0 + f)];
                    const Item &I = items[(size_t)cand[(size_t)at]];
                    S.push_back(I.S);
                    chunks.push_back(I.chunks);
                    cost += req[(size_t)at].bytes;
                    nj += verify ? (I.S + 15) / 16 + 2 * ((I.chunks + 15) / 16) : 2 * ((I.chunks + 15) / 16);
                    up += I.up_files;
                    expect(plan.ubase[(size_t)(G.item0 + f)] == terms, "a proof's first term");
                    terms += I.chunks;
                    if (f) expect(plan.order[(size_t)(G.item0 + f - 1)] < at, "input order inside a group");
                }
                expect(terms == G.units && cost == G.bytes, "the group's totals");
                // the ragged prefix sums
                std::vector<uint64_t> col0, slot0;
                const uint64_t cols = hb_mixed_prefix(S.data(), np, 1, col0);
                const uint64_t slots = hb_mixed_prefix(S.data(), np, 0, slot0);
                uint64_t want_cols = 0, want_slots = 0;
                for (uint64_t f = 0; f < np; ++f) {
                    expect(col0[(size_t)f] == want_cols && slot0[(size_t)f] == want_slots, "a proof's first column and slot");
                    want_cols += S[(size_t)f] + 1;
                    want_slots += S[(size_t)f];
                }
                expect(cols == want_cols && slots == want_slots, "the prefix sums end at the totals");
                if (verify) {
                    const HbArena L = hb_mverify_arena(z, rec, np, nj, terms, slots);
                    check_arena("verify arena", L,
                                {np * z.prf2, 3 * np * z.prf, np * z.vproof, np * rec, nj * HB_JOB_BYTES, slots * z.limbs,
                                 terms * z.limbs, terms * z.limbs, slots * z.limbs, np * z.limbs},
                                6, cost);
                    expect(L.n == HB_MXV_SECTIONS, "the enum names every section");
                    continue;
                }
                // the sum launch's table: one workgroup per (proof, column)
                std::vector<HbMxWg> sw((size_t)cols + 1, HbMxWg{~0u, ~0u});
                expect(hb_mixed_sum_wgs(S.data(), np, nullptr) == cols, "the count without a table");
                expect(hb_mixed_sum_wgs(S.data(), np, sw.data()) == cols, "one workgroup per column");
                expect(sw[(size_t)cols].proof == ~0u, "nothing written past the table");
                for (uint64_t w = 0; w < cols; ++w) {
                    const HbMxWg W = sw[(size_t)w];
                    expect(W.proof < np && W.a <= S[W.proof] && col0[W.proof] + W.a == w, "workgroup w is result column w");
                }
                // the conversion pass's table: every term exactly once, one proof per workgroup
                const uint64_t nmwg = hb_mixed_mont_wgs(chunks.data(), np, nullptr);
                std::vector<HbMxWg> mw((size_t)nmwg + 1, HbMxWg{~0u, ~0u});
                expect(hb_mixed_mont_wgs(chunks.data(), np, mw.data()) == nmwg, "the conversion table's count");
                expect(mw[(size_t)nmwg].proof == ~0u, "nothing written past the table");
                std::vector<uint8_t> hit((size_t)terms, 0);
                uint64_t want_wgs = 0;
                for (uint64_t f = 0; f < np; ++f) want_wgs += hb_mixed_mont_wg_count(chunks[(size_t)f]);
                expect(want_wgs == nmwg, "workgroups per proof add up");
                for (uint64_t w = 0; w < nmwg; ++w) {
                    const HbMxWg W = mw[(size_t)w];
                    expect(W.proof < np && W.a % HB_MX_MONT_TERMS == 0 && W.a < chunks[W.proof], "a workgroup starts inside its proof");
                    if (W.proof >= np) continue;
                    if (w) expect(mw[(size_t)w - 1].proof <= W.proof, "proofs in order");
                    for (uint32_t t = 0; t < HB_MX_MONT_TERMS; ++t) {
                        const uint64_t i = (uint64_t)W.a + t;
                        if (i >= chunks[W.proof]) break;   // the kernel's bound: the lane is idle, not another proof's
                        const uint64_t term = plan.ubase[(size_t)(G.item0 + W.proof)] + i;
                        expect(term < terms, "a term of the group");
                        if (term < terms) ++hit[(size_t)term];
                    }
                }
                for (uint64_t t = 0; t < terms; ++t) expect(hit[(size_t)t] == 1, "every term converted exactly once", (long long)t, hit[(size_t)t]);
                const HbArena L = hb_mprove_arena(z, rec, np, nj, cols, nmwg, up, terms);
                check_arena("prove arena", L,
                            {np * z.prf2, np * z.prf, np * z.pproof, np * rec, cols * HB_MXWG_BYTES, nmwg * HB_MXWG_BYTES,
                             nj * HB_JOB_BYTES, up, terms * 8, terms * z.limbs, cols * z.limbs},
                            8, cost);
                expect(L.n == HB_MXP_SECTIONS, "the enum names every section");
            }
            expect(placed == req.size(), "every proof in a group or through the single call");
        }
    }
}

// a pseudo-random odd number of `bits` bits, big-endian, with `lead` zero bytes in front
static std::vector<uint8_t> some_prime(int bits, uint64_t seed, size_t lead) {
    const size_t nb = (size_t)(bits + 7) / 8;
    std::vector<uint8_t> p(lead + nb, 0);
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 12345;
    for (size_t k = 0; k < nb; ++k) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        p[lead + k] = (uint8_t)(x >> 40);
    }
    const int top = bits - 8 * ((int)nb - 1);
    p[lead] = (uint8_t)((p[lead] & ((1u << top) - 1)) | (1u << (top - 1)));
    p[lead + nb - 1] |= 1;
    return p;
}

static void walk_cache() {
    static const int bits[] = {20, 61, 256, 257, 1000, 1024, 2048};
    HbPrimeCache cache;
    std::vector<std::vector<uint8_t>> primes;
    std::vector<size_t> entry;
    for (int k = 0; k < 7; ++k) primes.push_back(some_prime(bits[k], (uint64_t)k + 1, 0));
    // owners repeat: 40 positions over 7 primes, some spelt with leading zeros
    for (int pos = 0; pos < 40; ++pos) {
        const int k = (int)(rnd() % 7);
        const std::vector<uint8_t> spelt = some_prime(bits[k], (uint64_t)k + 1, rnd() % 3);
        const uint32_t nl = hb_mx_limbs(bits[k]);
        const size_t e = cache.get(spelt.data(), spelt.size(), nl);
        expect(e < cache.primes.size(), "an entry of the cache");
        const HbMxPrime &P = cache.primes[e];
        // the same constants for equal primes at different positions: recomputed here
        const hbhost::Limbs p = hbhost::from_be(primes[(size_t)k].data(), primes[(size_t)k].size(), nl);
        expect(P.nl == nl && P.p == p, "the entry is this prime's");
        expect(P.r2 == hbhost::pow2_mod(64u * nl, p), "R^2 mod p");
        expect(P.pinv == hbhost::mont_pinv(p[0]) && (uint32_t)(P.pinv * p[0]) == 0xffffffffu, "-1 / p mod 2^32");
        expect(P.inv_scaled == hbhost::inv_scaled(p), "the scaled 1 / p");
        expect(HbPrimeCache::key(spelt.data(), spelt.size()) == HbPrimeCache::key(primes[(size_t)k].data(), primes[(size_t)k].size()),
               "leading zeros do not change the key");
        entry.push_back(e);
    }
    expect(cache.primes.size() <= 7 && cache.misses == cache.primes.size(), "computed once per distinct prime",
           (long long)cache.misses);
    for (int a = 0; a < 7; ++a)
        for (int b = 0; b < a; ++b)
            expect(HbPrimeCache::key(primes[(size_t)a].data(), primes[(size_t)a].size()) !=
                       HbPrimeCache::key(primes[(size_t)b].data(), primes[(size_t)b].size()),
                   "distinct primes, distinct keys");
    expect(HbPrimeCache::key(nullptr, 0).empty(), "an empty prime has an empty key");
}

int main() {
    expect(hb_mx_limbs(8) == 8 && hb_mx_limbs(256) == 8 && hb_mx_limbs(257) == 16 && hb_mx_limbs(512) == 16 &&
               hb_mx_limbs(513) == 32 && hb_mx_limbs(1024) == 32 && hb_mx_limbs(1025) == 64 && hb_mx_limbs(2048) == 64 &&
               hb_mx_limbs(2049) == 0,
           "limb classes");
    expect(hb_mx_rounds(16) == 10 && hb_mx_rounds(24) == 12 && hb_mx_rounds(32) == 14 && hb_mx_rounds(15) == 0, "round counts");
    walk_mix(0, ~0ull, HB_BATCH_BYTES);
    for (int rep = 0; rep < 60; ++rep) {
        const uint64_t n = 1 + rnd() % 120;
        walk_mix(n, ~0ull, HB_BATCH_BYTES);           // one group per class
        walk_mix(n, 300, HB_BATCH_BYTES);             // the test switch's cap: several groups, long challenges through
        walk_mix(n, ~0ull, 20000 + rnd() % 200000);   // a small byte cap
    }
    walk_cache();
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
