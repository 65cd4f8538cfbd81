// Walks the host side of the cxx mixed-owner batches (hb_cxx_prove_mixed,
// hb_cxx_verify_rhs_mixed: the arena layouts and cost functions in
// heartbeat_amd/csrc/hb_mixed_host.hpp, planned by hb_cbatch_plan) over
// randomised mixes of primes, sector counts, key lengths, v_max widths and
// challenge lengths, as the runtime plans a class: the per-proof fall-through
// decision, the groups, every group's arena against the items' exact costs,
// the ragged column / alpha-slot prefix sums, the two workgroup tables and the
// wave-job queue.  Built with -fsanitize=address,undefined and run by
// tests/test_cxx_mixed_host.py.  Exit status 0 and "ok <n>" on success.
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

static uint64_t g_x = 0x2545f4914f6cdd1dull;
static uint64_t rnd() {
    g_x = g_x * 6364136223846793005ull + 1442695040888963407ull;
    return g_x >> 17;
}

struct Item {
    int bits;
    uint32_t nl, nr, chal_nr, S, tw, vnb;
    uint64_t chunks, range;   // the challenge's length; ntags (prove) / state_chunks (verify)
    uint64_t up_files;
    uint64_t eff() const { return chunks >= range ? range : chunks; }
    bool all() const { return chunks >= range; }
};

static Item some_item() {
    static const int bits[] = {61, 128, 256, 257, 384, 512, 1000, 1024, 2048};
    static const uint64_t counts[] = {0, 1, 63, 64, 65, 255, 256, 257, 600, 1000};
    static const uint32_t S[] = {1, 3, 10, 16, 40};
    static const uint64_t keys[] = {16, 24, 32};
    Item I;
    I.bits = bits[rnd() % 9];
    I.nl = hb_mx_limbs(I.bits);
    I.nr = hb_mx_rounds(keys[rnd() % 3]);
    I.chal_nr = rnd() % 8 ? I.nr : hb_mx_rounds(keys[rnd() % 3]);
    I.S = S[rnd() % 5];
    I.tw = (uint32_t)(I.bits + 7) / 8;
    I.vnb = rnd() % 6 ? I.tw : rnd() % 2 ? 16u : 5u;   // v_max = p mostly; 16 bytes; 5 bytes
    I.chunks = counts[rnd() % 10];
    I.range = 1 + counts[rnd() % 10];
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
    z.item = 24;
    z.cfile = 48;
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

// the runtime's request for one item (cxx_prove_mixed_impl / cxx_verify_mixed_impl)
static HbCbItemReq request(const Item &I, bool verify, const HbBatchSizes &z, uint64_t rec, uint64_t cap_bytes) {
    HbCbItemReq R = {};
    R.units = ~0ull;
    const uint64_t n = I.eff();
    const uint32_t vnb = verify && !n ? 16u : I.vnb;
    bool ok = I.tw % 16 == 0 && I.tw <= 4u * I.nl && vnb % 16 == 0;
    if (verify) {
        R.bytes = hb_cmverify_cost(z, rec, 2 * hb_cm_jobs(n) + hb_cm_jobs(I.S), n, I.S);
        ok = ok && I.nr == I.chal_nr;
    } else {
        R.bytes = hb_cmprove_cost(z, rec, (I.all() ? 1 : 2) * hb_cm_jobs(n), n, I.S, I.up_files);
    }
    if (!ok || R.bytes > cap_bytes) return R;
    R.n[HB_CB_V] = n;
    R.aes[HB_CB_V] = vnb / 16;
    if (verify) {
        R.n[HB_CB_IDXF] = n;
        R.n[HB_CB_ALPHA] = I.S;
        R.aes[HB_CB_IDXF] = R.aes[HB_CB_ALPHA] = I.tw / 16;
    } else {
        R.n[HB_CB_IDX] = I.all() ? 0 : n;
        R.aes[HB_CB_IDX] = 1;
    }
    R.units = n;
    return R;
}

static void walk_mix(uint64_t n, uint64_t cap_units, uint64_t cap_bytes) {
    std::vector<Item> items;
    std::vector<uint32_t> nl, nr;
    for (uint64_t i = 0; i < n; ++i) {
        items.push_back(some_item());
        nl.push_back(items.back().nl);
        nr.push_back(items.back().nr);
    }
    const std::vector<HbMxClass> classes = hb_mixed_partition(nl.data(), nr.data(), n);
    std::vector<int> seen((size_t)n, 0);
    for (const HbMxClass &K : classes)
        for (uint64_t i : K.items) ++seen[(size_t)i];
    for (uint64_t i = 0; i < n; ++i) expect(seen[(size_t)i] == 1, "every item in exactly one class", (long long)i);

    for (const HbMxClass &K : classes) {
        const HbBatchSizes z = sizes_of(K.nl);
        const uint64_t rec = rec_of(K.nl);
        for (int verify = 0; verify < 2; ++verify) {
            std::vector<HbCbItemReq> req;
            std::vector<uint64_t> cand;
            for (uint64_t i : K.items) {
                const Item &I = items[(size_t)i];
                if (!verify && I.eff() == 0) continue;   // the prove: zero sums, no descriptor in a group
                cand.push_back(i);
                req.push_back(request(I, verify != 0, z, rec, cap_bytes));
            }
            const uint64_t bound = cap_units < 0xffffffffull ? cap_units : 0xffffffffull;
            const HbCbPlan plan = hb_cbatch_plan(req.data(), req.size(), bound, cap_units, cap_bytes);
            // every item in exactly one group or in the fall-through list
            std::vector<int> placed(req.size(), 0);
            for (uint64_t k : plan.through) {
                expect(k < req.size(), "a fall-through item of the class");
                if (k < req.size()) ++placed[(size_t)k];
                expect(req[(size_t)k].units > bound, "only items over the bound fall through");
            }
            expect(plan.order.size() == plan.ubase.size(), "one first term per batched item");
            uint64_t next_job = 0;
            for (const HbCbGroup &G : plan.groups) {
                const uint64_t np = G.nitems;
                expect(np > 0 && G.item0 + np <= plan.order.size(), "a group's items");
                expect(G.job0 == next_job && G.job0 + G.njobs <= plan.jobs.size(), "a group's wave-jobs follow the last group's");
                next_job = G.job0 + G.njobs;
                std::vector<uint32_t> S, chunks;
                uint64_t cost = 0, nj = 0, up = 0, terms = 0;
                for (uint64_t f = 0; f < np; ++f) {
                    const uint64_t at = plan.order[(size_t)(G.item0 + f)];
                    ++placed[(size_t)at];
                    const Item &I = items[(size_t)cand[(size_t)at]];
                    const HbCbItemReq &R = req[(size_t)at];
                    expect(R.units == I.eff() && R.units <= bound, "a batched item is within the bound");
                    S.push_back(I.S);
                    chunks.push_back((uint32_t)I.eff());
                    cost += R.bytes;
                    for (uint32_t k = 0; k < HB_CB_KINDS; ++k) nj += hb_cm_jobs(R.n[k]);
                    up += verify ? 0 : I.up_files;
                    expect(plan.ubase[(size_t)(G.item0 + f)] == terms, "a proof's first term");
                    terms += I.eff();
                    if (f) expect(plan.order[(size_t)(G.item0 + f - 1)] < at, "input order inside a group");
                }
                expect(terms == G.units && cost == G.bytes, "the group's totals");
                expect(nj == G.njobs, "the group's wave-jobs are its items'", (long long)nj, (long long)G.njobs);
                if (np > 1) expect(G.units <= cap_units && G.bytes <= cap_bytes, "a group of several stays under the caps");
                // the queue: every evaluation of every item and kind exactly once, longest first
                std::vector<std::vector<uint8_t>> hit((size_t)np * HB_CB_KINDS);
                for (uint64_t f = 0; f < np; ++f)
                    for (uint32_t k = 0; k < HB_CB_KINDS; ++k)
                        hit[(size_t)(f * HB_CB_KINDS + k)].assign((size_t)req[(size_t)plan.order[(size_t)(G.item0 + f)]].n[k], 0);
                uint32_t last_aes = ~0u;
                for (uint64_t j = G.job0; j < G.job0 + G.njobs; ++j) {
                    const HbCbJob &Jb = plan.jobs[(size_t)j];
                    expect(Jb.item < np && Jb.kind < HB_CB_KINDS && Jb.count >= 1 && Jb.count <= HB_CB_JOB, "a wave-job of the group");
                    if (Jb.item >= np || Jb.kind >= HB_CB_KINDS) continue;
                    const HbCbItemReq &R = req[(size_t)plan.order[(size_t)(G.item0 + Jb.item)]];
                    expect((uint64_t)Jb.first + Jb.count <= R.n[Jb.kind], "inside the item's evaluations");
                    expect(R.aes[Jb.kind] >= 1 && R.aes[Jb.kind] <= last_aes, "longest tries first");
                    last_aes = R.aes[Jb.kind];
                    std::vector<uint8_t> &h = hit[(size_t)(Jb.item * HB_CB_KINDS + Jb.kind)];
                    for (uint32_t t = 0; t < Jb.count && (uint64_t)Jb.first + t < h.size(); ++t) ++h[(size_t)Jb.first + t];
                }
                for (const std::vector<uint8_t> &h : hit)
                    for (uint8_t c : h) expect(c == 1, "every evaluation in exactly one wave-job", c);
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
                    const HbArena L = hb_cmverify_arena(z, rec, np, nj, terms, slots);
                    check_arena("cxx verify arena", L,
                                {np * z.prf2, 3 * np * z.prf, np * z.item, np * z.vproof, np * rec, nj * HB_JOB_BYTES,
                                 slots * z.limbs, terms * z.limbs, terms * z.limbs, slots * z.limbs, np * z.limbs},
                                7, cost);
                    expect(L.n == HB_CMV_SECTIONS, "the enum names every section");
                    expect(L.off[HB_CMV_RES] + np * z.limbs == L.total, "the results end the arena");
                    continue;
                }
                // the sum launch's table: one workgroup per (proof, column)
                std::vector<HbMxWg> sw((size_t)cols + 1, HbMxWg{~0u, ~0u});
                expect(hb_mixed_sum_wgs(S.data(), np, sw.data()) == cols, "one workgroup per column");
                expect(sw[(size_t)cols].proof == ~0u, "nothing written past the table");
                for (uint64_t w = 0; w < cols; ++w) {
                    const HbMxWg W = sw[(size_t)w];
                    expect(W.proof < np && W.a <= S[W.proof] && col0[W.proof] + W.a == w, "workgroup w is result column w");
                }
                // the conversion pass's table over the EFFECTIVE chunk counts: every term exactly once
                const uint64_t nmwg = hb_mixed_mont_wgs(chunks.data(), np, nullptr);
                std::vector<HbMxWg> mw((size_t)nmwg + 1, HbMxWg{~0u, ~0u});
                expect(hb_mixed_mont_wgs(chunks.data(), np, mw.data()) == nmwg, "the conversion table's count");
                expect(mw[(size_t)nmwg].proof == ~0u, "nothing written past the table");
                std::vector<uint8_t> conv((size_t)terms, 0);
                for (uint64_t w = 0; w < nmwg; ++w) {
                    const HbMxWg W = mw[(size_t)w];
                    expect(W.proof < np && W.a % HB_MX_MONT_TERMS == 0 && W.a < chunks[W.proof], "a workgroup starts inside its proof");
                    if (W.proof >= np) continue;
                    for (uint32_t t = 0; t < HB_MX_MONT_TERMS; ++t) {
                        const uint64_t i = (uint64_t)W.a + t;
                        if (i >= chunks[W.proof]) break;   // the kernel's bound
                        const uint64_t term = plan.ubase[(size_t)(G.item0 + W.proof)] + i;
                        expect(term < terms, "a term of the group");
                        if (term < terms) ++conv[(size_t)term];
                    }
                }
                for (uint64_t t = 0; t < terms; ++t) expect(conv[(size_t)t] == 1, "every term converted exactly once", (long long)t);
                const HbArena L = hb_cmprove_arena(z, rec, np, nj, cols, nmwg, up, terms);
                check_arena("cxx prove arena", L,
                            {np * z.prf2, np * z.prf, np * z.item, np * z.pproof, np * rec, cols * HB_MXWG_BYTES,
                             nmwg * HB_MXWG_BYTES, nj * HB_JOB_BYTES, up, terms * 8, terms * z.limbs, cols * z.limbs, np * 4},
                            9, cost);
                expect(L.n == HB_CMP_SECTIONS && L.n <= HbArena::kMaxSections, "the enum names every section");
                // results and status words come back in one copy
                expect(L.off[HB_CMP_STATUS] >= L.off[HB_CMP_RES] + cols * z.limbs && L.off[HB_CMP_STATUS] + np * 4 == L.total,
                       "the status words follow the results and end the arena");
            }
            expect(next_job == plan.jobs.size(), "no wave-job outside a group");
            for (size_t k = 0; k < placed.size(); ++k)
                expect(placed[k] == 1, "every item in exactly one group or in the fall-through list", (long long)k, placed[k]);
        }
    }
}

int main() {
    expect(hb_cm_jobs(0) == 0 && hb_cm_jobs(1) == 1 && hb_cm_jobs(HB_CB_JOB) == 1 && hb_cm_jobs(HB_CB_JOB + 1) == 2, "wave-jobs of n");
    walk_mix(0, ~0ull, HB_BATCH_BYTES);
    for (int rep = 0; rep < 60; ++rep) {
        const uint64_t n = 1 + rnd() % 120;
        walk_mix(n, ~0ull, HB_BATCH_BYTES);           // one group per class
        walk_mix(n, 300, HB_BATCH_BYTES);             // the test switch's cap: several groups, long challenges through
        walk_mix(n, ~0ull, 20000 + rnd() % 200000);   // a small byte cap: items alone above it fall through
    }
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
