// Walks the pure host header of the mixed-owner encodes
// (heartbeat_amd/csrc/hb_emixed_host.hpp) over randomised mixes of primes,
// sector counts (1 .. T + 1 and beyond), key lengths and file lengths (empty
// files, files that end on a block boundary, thousands of files): the grouping
// of each class with the mixed encode's costs, every group's arena against the
// files' costs, the alpha-slot prefix sums and F-buffer bases, the PySwizzle
// side's wave-job table, both workgroup tables (the MAC launches' and the
// conversion pass's) and a host model of the kernels' index arithmetic over
// them: every block tagged exactly once, every alpha slot converted exactly
// once, nothing read or written outside the group's buffers.  Built with
// -fsanitize=address,undefined and run by tests/test_encode_mixed_host.py.
// Exit status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hb_emixed_host.hpp"

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
    uint32_t nl, nr, S, ss, tw;
    uint64_t len;
};

static uint32_t threads_of(uint32_t nl) { return nl >= 64 ? 128u : 256u; }   // HbMacSplit<NL>::T

static Item some_item(bool small) {
    static const int bits[] = {20, 61, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025, 2048};
    static const uint64_t keys[] = {16, 24, 32};
    Item I;
    I.bits = bits[rnd() % 12];
    I.nl = hb_mx_limbs(I.bits);
    I.nr = hb_mx_rounds(keys[rnd() % 3]);
    I.ss = (uint32_t)I.bits / 8;
    I.tw = (uint32_t)(I.bits + 7) / 8;
    const uint32_t T = threads_of(I.nl);
    static const uint32_t fixed[] = {1, 2, 3, 10, 15, 16, 17, 40, 255, 256, 257};
    switch (rnd() % 4) {
    case 0: I.S = 1 + (uint32_t)(rnd() % (T + 1)); break;          // 1 .. T + 1
    case 1: I.S = T - 1 + (uint32_t)(rnd() % 3); break;            // T - 1, T, T + 1
    default: I.S = fixed[rnd() % 11]; break;
    }
    const uint64_t C = (uint64_t)I.ss * I.S;
    switch (rnd() % 6) {
    case 0: I.len = 0; break;
    case 1: I.len = C * (rnd() % 4); break;                         // ends on a block boundary
    case 2: I.len = C * (T / (I.S <= T ? I.S : 1) + rnd() % 2) + rnd() % 3; break;   // crosses a MAC workgroup
    default: I.len = rnd() % (small ? 2000 : 40 * C + 1); break;
    }
    return I;
}

// sizes as the runtime's batch_sizes<NL>() has them, to the rounding
static HbBatchSizes sizes_of(uint32_t nl) {
    HbBatchSizes z = {};
    z.prf2 = 60 * 4 + 2 * 4 + 24;
    z.prf = 60 * 4 + nl * 4 + 24;
    z.limbs = nl * 4;
    z.file = 40;
    z.wg = 8;
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
    expect(sum == cost, "the sections are exactly what the files cost", (long long)sum, (long long)cost);
    expect(L.total <= cost + 16 * (uint64_t)L.n, "total <= costs + 16 x sections", (long long)L.total, (long long)cost);
}

static void walk_mix(uint64_t n, uint64_t cap_units, uint64_t cap_bytes, bool small) {
    std::vector<Item> items;
    std::vector<uint32_t> nl, nr;
    for (uint64_t i = 0; i < n; ++i) {
        items.push_back(some_item(small));
        nl.push_back(items.back().nl);
        nr.push_back(items.back().nr);
    }
    uint64_t in_class = 0;
    for (const HbMxClass &K : hb_mixed_partition(nl.data(), nr.data(), n)) {
        in_class += K.items.size();
        const HbBatchSizes z = sizes_of(K.nl);
        const uint64_t rec = rec_of(K.nl);
        const uint32_t T = threads_of(K.nl);
        for (int cxx = 0; cxx < 2; ++cxx) {
            auto blocks_of = [&](const Item &I) { return I.len / ((uint64_t)I.ss * I.S) + 1; };
            auto mac_blocks_of = [&](const Item &I) {
                const uint64_t C = (uint64_t)I.ss * I.S;
                return cxx ? I.len / C + (I.len % C ? 1 : 0) : blocks_of(I);
            };
            auto jobs_of = [&](const Item &I) {
                return cxx ? hb_cm_jobs(blocks_of(I)) + hb_cm_jobs(I.S) : hb_em_job_count(I.S, blocks_of(I));
            };
            std::vector<HbCbItemReq> req;
            for (uint64_t i : K.items) {
                const Item &I = items[(size_t)i];
                HbCbItemReq R = {};
                R.n[HB_CB_F] = blocks_of(I);
                R.n[HB_CB_ALPHA] = I.S;
                R.aes[HB_CB_F] = R.aes[HB_CB_ALPHA] = I.tw / 16;
                R.units = blocks_of(I);
                R.bytes = hb_em_cost(z, rec, jobs_of(I), hb_em_mac_wg_count(T, I.S, mac_blocks_of(I)), hb_up16(I.len), blocks_of(I),
                                     I.S, hb_up16(blocks_of(I) * I.tw));
                req.push_back(R);
            }
            const HbCbPlan plan = cxx ? hb_cbatch_plan(req.data(), req.size(), cap_units, cap_units, cap_bytes)
                                      : hb_batch_groups(req.data(), req.size(), cap_units, cap_units, cap_bytes);
            uint64_t placed = plan.through.size();
            for (const HbCbGroup &G : plan.groups) {
                placed += G.nitems;
                const uint64_t nf = G.nitems;
                std::vector<uint32_t> S;
                std::vector<uint64_t> nb, mb;
                uint64_t cost = 0, dbytes = 0, tbytes = 0, nj_cxx = 0;
                for (uint64_t f = 0; f < nf; ++f) {
                    const uint64_t at = plan.order[(size_t)(G.item0 + f)];
                    const Item &I = items[(size_t)K.items[(size_t)at]];
                    S.push_back(I.S);
                    nb.push_back(blocks_of(I));
                    mb.push_back(mac_blocks_of(I));
                    cost += req[(size_t)at].bytes;
                    dbytes += hb_up16(I.len);
                    tbytes += hb_up16(blocks_of(I) * I.tw);
                    nj_cxx += jobs_of(I);
                }
                // ---- prefix sums: alpha slots and F bases
                std::vector<uint64_t> slot0, fbase;
                const uint64_t slots = hb_mixed_prefix(S.data(), nf, 0, slot0);
                const uint64_t blocks = hb_em_fbases(nb.data(), nf, fbase);
                expect(blocks == G.units, "the group's blocks", (long long)blocks, (long long)G.units);
                uint64_t ws = 0, wb = 0;
                for (uint64_t f = 0; f < nf; ++f) {
                    expect(slot0[(size_t)f] == ws && fbase[(size_t)f] == wb, "a file's first slot and first block");
                    expect(fbase[(size_t)f] == plan.ubase[(size_t)(G.item0 + f)], "the F base is the planner's unit base");
                    ws += S[(size_t)f];
                    wb += nb[(size_t)f];
                }
                expect(ws == slots && wb == blocks, "the prefix sums end at the totals");
                // ---- the wave-job table (PySwizzle side): every evaluation once, alpha directly before F
                uint64_t nj = nj_cxx;
                if (!cxx) {
                    nj = hb_em_jobs(S.data(), nb.data(), nf, nullptr);
                    std::vector<HbEmJob> jobs((size_t)nj + 1, HbEmJob{~0u, ~0u, ~0u, ~0u});
                    expect(hb_em_jobs(S.data(), nb.data(), nf, jobs.data()) == nj, "the job table's count");
                    expect(jobs[(size_t)nj].file == ~0u, "nothing written past the job table");
                    std::vector<uint8_t> hitf((size_t)blocks, 0), hita((size_t)slots, 0);
                    uint64_t want = 0;
                    for (uint64_t f = 0; f < nf; ++f) want += hb_em_job_count(S[(size_t)f], nb[(size_t)f]);
                    expect(want == nj, "jobs per file add up");
                    for (uint64_t j = 0; j < nj; ++j) {
                        const HbEmJob J = jobs[(size_t)j];
                        expect(J.file < nf && J.kind <= 1 && J.count >= 1 && J.count <= 16 && J.first % 16 == 0, "a wave-job's shape");
                        if (J.file >= nf) continue;
                        if (j) {
                            const HbEmJob P = jobs[(size_t)j - 1];
                            expect(P.file < J.file || (P.file == J.file && (P.kind > J.kind || (P.kind == J.kind && P.first < J.first))),
                                   "files in order, alpha before F, evaluations ascending");
                        }
                        const uint64_t lim = J.kind ? S[J.file] : nb[J.file];
                        expect((uint64_t)J.first + J.count <= lim, "inside the file's evaluations");
                        for (uint32_t e = 0; e < J.count && (uint64_t)J.first + e < lim; ++e) {
                            if (J.kind) ++hita[(size_t)(slot0[J.file] + J.first + e)];
                            else ++hitf[(size_t)(fbase[J.file] + J.first + e)];
                        }
                    }
                    for (uint64_t t = 0; t < blocks; ++t) expect(hitf[(size_t)t] == 1, "every F evaluated once", (long long)t);
                    for (uint64_t t = 0; t < slots; ++t) expect(hita[(size_t)t] == 1, "every alpha evaluated once", (long long)t);
                }
                // ---- the MAC launches' table: the kernels' block index over it
                uint64_t nsplit = ~0ull, nsplit2 = ~0ull;
                const uint64_t nwg = hb_em_mac_wgs(S.data(), mb.data(), nf, T, nullptr, &nsplit);
                std::vector<HbEmWg> wgs((size_t)nwg + 1, HbEmWg{~0u, ~0u});
                expect(hb_em_mac_wgs(S.data(), mb.data(), nf, T, wgs.data(), &nsplit2) == nwg && nsplit == nsplit2 && nsplit <= nwg,
                       "the MAC table's counts");
                expect(wgs[(size_t)nwg].file == ~0u, "nothing written past the MAC table");
                uint64_t want_wgs = 0;
                for (uint64_t f = 0; f < nf; ++f) want_wgs += hb_em_mac_wg_count(T, S[(size_t)f], mb[(size_t)f]);
                expect(want_wgs == nwg, "workgroups per file add up");
                std::vector<uint8_t> tagged((size_t)blocks, 0);
                for (uint64_t w = 0; w < nwg; ++w) {
                    const HbEmWg W = wgs[(size_t)w];
                    expect(W.file < nf, "a file of the group");
                    if (W.file >= nf) continue;
                    const uint32_t Sf = S[W.file];
                    const bool split = w < nsplit;
                    expect(split == hb_em_split(T, Sf), "a workgroup in its shape's launch", (long long)w, Sf);
                    expect(W.first < mb[W.file] && W.first % hb_em_bpw(T, Sf) == 0, "a workgroup starts inside its file");
                    if (split) {
                        // hb_emixed_mac_split_kernel: T lanes, lb = lane / S, j = lane % S
                        const uint32_t bpw = T / Sf;
                        expect(bpw >= 1 && bpw * Sf <= T, "the live lanes fit the workgroup");
                        for (uint32_t lane = 0; lane < T; ++lane) {
                            const uint32_t lb = lane / Sf, j = lane % Sf;
                            const uint64_t k = (uint64_t)W.first + lb;
                            if (!(lb < bpw && k < mb[W.file])) continue;
                            expect(slot0[W.file] + j < slots, "alpha slot inside the group's");
                            expect((uint64_t)lane + (j == 0 ? Sf - 1 : 0) < T, "the reduction reads inside the LDS array");
                            if (j == 0) ++tagged[(size_t)(fbase[W.file] + k)];
                        }
                    } else {
                        // hb_emixed_mac_lane_kernel: 256 lanes, a block each
                        for (uint32_t lane = 0; lane < HB_EM_LANE_BLOCKS; ++lane) {
                            const uint64_t k = (uint64_t)W.first + lane;
                            if (k >= mb[W.file]) break;
                            ++tagged[(size_t)(fbase[W.file] + k)];
                        }
                    }
                }
                for (uint64_t f = 0; f < nf; ++f)
                    for (uint64_t k = 0; k < nb[(size_t)f]; ++k)
                        expect(tagged[(size_t)(fbase[(size_t)f] + k)] == (k < mb[(size_t)f] ? 1 : 0),
                               "every MAC block tagged exactly once, the no-sector block never", (long long)f, (long long)k);
                // ---- the conversion pass's table over the alpha slots
                const uint64_t nmwg = hb_mixed_mont_wgs(S.data(), nf, nullptr);
                std::vector<HbMxWg> mw((size_t)nmwg + 1, HbMxWg{~0u, ~0u});
                expect(hb_mixed_mont_wgs(S.data(), nf, mw.data()) == nmwg, "the conversion table's count");
                expect(mw[(size_t)nmwg].proof == ~0u, "nothing written past the conversion table");
                std::vector<uint8_t> conv((size_t)slots, 0);
                for (uint64_t w = 0; w < nmwg; ++w) {
                    const HbMxWg W = mw[(size_t)w];
                    expect(W.proof < nf && W.a < S[W.proof < nf ? W.proof : 0], "a conversion workgroup starts inside its file");
                    if (W.proof >= nf) continue;
                    for (uint32_t t = 0; t < HB_MX_MONT_TERMS; ++t) {
                        const uint64_t i = (uint64_t)W.a + t;
                        if (i >= S[W.proof]) break;
                        ++conv[(size_t)(slot0[W.proof] + i)];
                    }
                }
                for (uint64_t t = 0; t < slots; ++t) expect(conv[(size_t)t] == 1, "every alpha slot converted exactly once", (long long)t);
                // ---- the arena
                const HbArena L = hb_em_arena(z, rec, nf, nj, nwg, nmwg, dbytes, blocks, slots, tbytes);
                check_arena(cxx ? "cxx encode arena" : "encode arena", L,
                            {2 * nf * z.prf, nf * z.file, nf * rec, nf * z.pproof, nj * HB_JOB_BYTES, nwg * HB_EMWG_BYTES,
                             nmwg * HB_MXWG_BYTES, dbytes, blocks * z.limbs, slots * z.limbs, tbytes},
                            8, cost);
                expect(L.n == HB_EMX_SECTIONS, "the enum names every section");
            }
            expect(placed == req.size(), "every file in a group or through the single call");
        }
    }
    expect(in_class == n, "every file in a class");
}

int main() {
    expect(hb_em_bpw(256, 1) == 256 && hb_em_bpw(256, 2) == 128 && hb_em_bpw(256, 10) == 25 && hb_em_bpw(256, 255) == 1 &&
               hb_em_bpw(256, 256) == 1 && hb_em_bpw(256, 257) == 256 && hb_em_bpw(128, 128) == 1 && hb_em_bpw(128, 129) == 256,
           "blocks per workgroup at the shapes' boundaries");
    expect(!hb_em_split(256, 1) && hb_em_split(256, 2) && hb_em_split(256, 256) && !hb_em_split(256, 257) &&
               hb_em_split(128, 128) && !hb_em_split(128, 129),
           "the shapes' boundaries");
    expect(hb_em_job_count(1, 1) == 2 && hb_em_job_count(16, 16) == 2 && hb_em_job_count(17, 17) == 4, "wave-jobs at 16 / 17");
    walk_mix(0, ~0ull, HB_BATCH_BYTES, true);
    for (int rep = 0; rep < 40; ++rep) {
        const uint64_t n = 1 + rnd() % 60;
        walk_mix(n, ~0ull, HB_BATCH_BYTES, false);          // one group per class
        walk_mix(n, 40, HB_BATCH_BYTES, false);             // the test switch's cap: several groups, long files through
        walk_mix(n, ~0ull, 20000 + rnd() % 200000, false);  // a small byte cap
    }
    walk_mix(5000, ~0ull, HB_BATCH_BYTES, true);            // thousands of small files
    walk_mix(3000, 7, HB_BATCH_BYTES, true);
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
