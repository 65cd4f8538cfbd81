// Walks hb_cbatch_plan (heartbeat_amd/csrc/hb_cbatch_plan.hpp) through the
// cases of the batched cxx calls' planner; built with
// -fsanitize=address,undefined and run by tests/test_cbatch_plan.py.  Exit
// status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <utility>
#include <vector>

#include "hb_cbatch_plan.hpp"

static int g_checks = 0, g_bad = 0;

static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    ++g_checks;
    if (!ok) {
        ++g_bad;
        printf("FAIL %s (%lld, %lld)\n", what, a, b);
    }
}

static HbCbItemReq item(uint64_t nf, uint64_t na, uint32_t aes_f, uint32_t aes_a, uint64_t bytes) {
    HbCbItemReq R = {};
    R.n[HB_CB_F] = nf;
    R.n[HB_CB_ALPHA] = na;
    R.aes[HB_CB_F] = aes_f;
    R.aes[HB_CB_ALPHA] = aes_a;
    R.units = nf;
    R.bytes = bytes;
    return R;
}

// What every plan must satisfy: each item either falls through or sits in
// exactly one group, in the caller's order; every evaluation of a batched
// item is covered by exactly one wave-job of its group and no wave-job holds
// more than HB_CB_JOB or none; a group's queue is longest first; ubase is the
// running sum of units; a group of more than one item respects the caps.
static void check_plan(const char *what, const std::vector<HbCbItemReq> &it, const HbCbPlan &P, uint64_t bound,
                       uint64_t cap_units, uint64_t cap_bytes) {
    std::vector<int> seen(it.size(), 0);
    for (uint64_t i : P.through) {
        expect(i < it.size() && it[i].units > bound, "through item is over the bound", (long long)i);
        if (i < it.size()) ++seen[i];
    }
    for (size_t k = 1; k < P.through.size(); ++k) expect(P.through[k - 1] < P.through[k], "through keeps the order");
    expect(P.order.size() == P.ubase.size(), "order and ubase have one length");
    uint64_t next_item = 0, next_job = 0;
    for (const HbCbGroup &G : P.groups) {
        expect(G.nitems > 0, what);
        expect(G.item0 == next_item && G.job0 == next_job, "groups are contiguous");
        next_item = G.item0 + G.nitems;
        next_job = G.job0 + G.njobs;
        if (next_item > P.order.size() || next_job > P.jobs.size()) {
            expect(false, "group inside the tables");
            return;
        }
        uint64_t units = 0, bytes = 0;
        std::map<std::pair<uint32_t, uint32_t>, std::vector<char>> cover;
        for (uint64_t f = 0; f < G.nitems; ++f) {
            const uint64_t i = P.order[G.item0 + f];
            expect(i < it.size() && it[i].units <= bound, "batched item is under the bound", (long long)i);
            if (i >= it.size()) return;
            if (f) expect(P.order[G.item0 + f - 1] < i, "a group keeps the order");
            ++seen[i];
            expect(P.ubase[G.item0 + f] == units, "ubase is the running sum", (long long)i);
            units += it[i].units;
            bytes += it[i].bytes;
            for (uint32_t k = 0; k < HB_CB_KINDS; ++k) cover[{(uint32_t)f, k}].assign((size_t)it[i].n[k], 0);
        }
        expect(units == G.units && bytes == G.bytes, "group totals");
        if (G.nitems > 1) expect(units <= cap_units && bytes <= cap_bytes, "caps respected", (long long)units, (long long)bytes);
        uint64_t prev_len = ~0ull, prev_count = ~0ull;
        for (uint64_t j = 0; j < G.njobs; ++j) {
            const HbCbJob &J = P.jobs[G.job0 + j];
            expect(J.item < G.nitems && J.kind < HB_CB_KINDS, "job names an item of its group");
            if (J.item >= G.nitems || J.kind >= HB_CB_KINDS) return;
            expect(J.count >= 1 && J.count <= HB_CB_JOB, "1 <= count <= HB_CB_JOB", J.count);
            std::vector<char> &c = cover[{J.item, J.kind}];
            expect((uint64_t)J.first + J.count <= c.size(), "job inside its item", J.first, J.count);
            if ((uint64_t)J.first + J.count > c.size()) return;
            for (uint32_t e = 0; e < J.count; ++e) {
                expect(!c[J.first + e], "evaluation covered once", J.first + e);
                c[J.first + e] = 1;
            }
            const uint64_t len = it[P.order[G.item0 + J.item]].aes[J.kind];
            expect(len < prev_len || (len == prev_len && J.count <= prev_count), "longest first", (long long)len,
                   (long long)prev_len);
            prev_len = len;
            prev_count = J.count;
        }
        for (auto &kv : cover)
            for (char x : kv.second) expect(x != 0, "no evaluation missed");
    }
    expect(next_item == P.order.size() && next_job == P.jobs.size(), "groups cover the tables");
    for (size_t i = 0; i < it.size(); ++i) expect(seen[i] == 1, "every item exactly once", (long long)i);
}

static HbCbPlan run(const char *what, const std::vector<HbCbItemReq> &it, uint64_t bound, uint64_t cap_units,
                    uint64_t cap_bytes) {
    HbCbPlan P = hb_cbatch_plan(it.data(), it.size(), bound, cap_units, cap_bytes);
    check_plan(what, it, P, bound, cap_units, cap_bytes);
    return P;
}

static uint64_t jobs_of_kind(const HbCbPlan &P, uint32_t item, uint32_t kind) {
    uint64_t n = 0;
    for (const HbCbJob &J : P.jobs) n += J.item == item && J.kind == kind;
    return n;
}

int main() {
    const uint64_t BIG = ~0ull, J = HB_CB_JOB;

    {   // no items, and a null table of none
        HbCbPlan P = hb_cbatch_plan(nullptr, 0, BIG, BIG, BIG);
        expect(P.groups.empty() && P.jobs.empty() && P.order.empty() && P.through.empty(), "empty batch");
    }
    {   // wave-job boundaries at HB_CB_JOB +- 1
        std::vector<HbCbItemReq> it = {item(J - 1, 1, 8, 8, 100), item(J, J, 8, 8, 100), item(J + 1, J + 1, 8, 8, 100),
                                       item(4 * J + 1, 10, 8, 8, 100), item(1, 1, 8, 8, 100)};
        HbCbPlan P = run("boundaries", it, BIG, BIG, BIG);
        expect(P.groups.size() == 1 && P.through.empty(), "one group");
        expect(jobs_of_kind(P, 0, HB_CB_F) == 1 && jobs_of_kind(P, 1, HB_CB_F) == 1, "J - 1 and J: one wave-job");
        expect(jobs_of_kind(P, 2, HB_CB_F) == 2 && jobs_of_kind(P, 2, HB_CB_ALPHA) == 2, "J + 1: two wave-jobs");
        expect(jobs_of_kind(P, 3, HB_CB_F) == 5, "4 J + 1: five wave-jobs");
        expect(P.jobs.size() == 1 + 1 + 1 + 1 + 2 + 2 + 5 + 1 + 1 + 1, "job count", (long long)P.jobs.size());
        expect(P.jobs.front().count == J && P.jobs.back().count == 1, "full wave-jobs first at equal length");
    }
    {   // longest first over kinds of unequal length, items of unequal length
        std::vector<HbCbItemReq> it = {item(70, 10, 2, 8, 1), item(3, 200, 4, 1, 1), item(64, 64, 8, 2, 1)};
        HbCbPlan P = run("lengths", it, BIG, BIG, BIG);
        expect(P.jobs.front().kind == HB_CB_F && P.jobs.front().item == 2 && P.jobs[1].kind == HB_CB_ALPHA &&
                   P.jobs[1].item == 0,
               "the 8-block tries first, the fuller wave-job before the other");
        expect(P.jobs.back().kind == HB_CB_ALPHA && P.jobs.back().item == 1 && P.jobs.back().count == 200 - 3 * J,
               "the short tail of the shortest kind is last");
    }
    {   // items without evaluations get no jobs but belong to a group
        std::vector<HbCbItemReq> it = {item(0, 0, 8, 8, 10), item(5, 0, 8, 8, 10), item(0, 3, 8, 8, 10)};
        HbCbPlan P = run("no evaluations", it, BIG, BIG, BIG);
        expect(P.groups.size() == 1 && P.order.size() == 3, "all three batched");
        expect(jobs_of_kind(P, 0, HB_CB_F) + jobs_of_kind(P, 0, HB_CB_ALPHA) == 0, "item 0 has no wave-job");
        expect(jobs_of_kind(P, 1, HB_CB_ALPHA) == 0 && jobs_of_kind(P, 2, HB_CB_F) == 0, "empty kinds have none");
        expect(P.jobs.size() == 2, "two wave-jobs");
    }
    {   // the unit cap: seven items, cap 20, one over the bound
        std::vector<HbCbItemReq> it;
        for (int i = 0; i < 7; ++i) it.push_back(item(i == 2 ? 50 : 10, 2, 8, 8, 100));
        HbCbPlan P = run("unit cap", it, 20, 20, BIG);
        expect(P.groups.size() == 3 && P.through.size() == 1 && P.through[0] == 2, "three groups, item 2 falls through");
        for (const HbCbGroup &G : P.groups) expect(G.nitems == 2 && G.units == 20, "two items per group");
        expect(P.order[2] == 3 && P.ubase[3] == 10, "the group after the skipped item");
    }
    {   // the byte cap, with one oversized item that gets a group of its own
        std::vector<HbCbItemReq> it = {item(1, 1, 8, 8, 400), item(1, 1, 8, 8, 400), item(1, 1, 8, 8, 5000),
                                       item(1, 1, 8, 8, 300), item(1, 1, 8, 8, 700), item(1, 1, 8, 8, 1)};
        HbCbPlan P = run("byte cap", it, BIG, BIG, 1000);
        expect(P.groups.size() == 4, "four groups", (long long)P.groups.size());
        if (P.groups.size() == 4) {
            expect(P.groups[0].nitems == 2 && P.groups[0].bytes == 800, "400 + 400");
            expect(P.groups[1].nitems == 1 && P.groups[1].bytes == 5000, "the oversized item alone");
            expect(P.groups[2].nitems == 2 && P.groups[2].bytes == 1000, "300 + 700 just fits");
            expect(P.groups[3].nitems == 1 && P.groups[3].bytes == 1, "one byte more starts a group");
        }
    }
    {   // everything falls through; bound 0
        std::vector<HbCbItemReq> it = {item(5, 1, 8, 8, 1), item(6, 1, 8, 8, 1)};
        HbCbPlan P = run("all through", it, 4, BIG, BIG);
        expect(P.groups.empty() && P.jobs.empty() && P.through.size() == 2, "no group");
        it.push_back(item(0, 1, 8, 8, 1));
        P = run("bound 0", it, 0, BIG, BIG);
        expect(P.groups.size() == 1 && P.order.size() == 1 && P.order[0] == 2, "only the item without units is batched");
    }
    {   // sizes near 2^64: no overflow in the cap arithmetic
        std::vector<HbCbItemReq> it = {item(3, 1, 8, 8, BIG - 5), item(3, 1, 8, 8, 10), item(3, 1, 8, 8, BIG)};
        HbCbPlan P = run("huge bytes", it, BIG, BIG, BIG - 1);
        expect(P.groups.size() == 3, "each alone");
        const uint64_t M = (1ull << 20) + 1;
        std::vector<HbCbItemReq> big = {item(M, 0, 1, 1, 1)};
        big[0].units = BIG;
        P = run("units over the caps, alone", big, BIG, 7, 7);
        expect(P.groups.size() == 1 && P.jobs.size() == (M + J - 1) / J, "2^20 + 1 evaluations");
        expect(P.jobs.back().first + (uint64_t)P.jobs.back().count == M && P.jobs.back().count == 1,
               "the last wave-job ends the item");
    }
    {   // many items in several groups: the invariants at scale
        std::vector<HbCbItemReq> it;
        uint64_t x = 12345;
        for (int i = 0; i < 500; ++i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            it.push_back(item((x >> 33) % 300, (x >> 20) % 130, 1 + (uint32_t)((x >> 10) % 16), 1 + (uint32_t)((x >> 5) % 16),
                              (x >> 40) % 9000));
        }
        HbCbPlan P = run("random", it, 250, 1000, 20000);
        expect(P.groups.size() > 10 && !P.through.empty(), "several groups and fall-throughs");
    }

    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
