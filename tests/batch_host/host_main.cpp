// Walks the pure host header of the batched calls
// (heartbeat_amd/csrc/hb_batch_host.hpp): the six calls' arena layouts against
// their cost functions, the shared grouping against a transcription of the
// greedy loop it replaced, and the limb conversions against the hand loops
// they replaced.  Built with -fsanitize=address,undefined and run by
// tests/test_batch_host.py.  Exit status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hb_batch_host.hpp"

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

// sizes an item can have: the edges of the 16-byte rounding, ordinary ones,
// and (big) values near 2^32
static uint64_t some_size(bool big) {
    static const uint64_t edge[] = {0, 1, 15, 16, 17, 31, 32, 33, 95, 200};
    const uint64_t k = rnd() % 16;
    if (k < 10) return edge[k];
    if (big && k == 10) return (1ull << 32) - 1 - rnd() % 40;
    if (big && k == 11) return (1ull << 32) + rnd() % 40;
    return rnd() % 5000;
}

// What every layout must satisfy.  sizes: the sections' byte sizes in order,
// n_up of them uploaded; cost: the sum of the items' costs.
static void check_arena(const char *what, const HbArena &L, const std::vector<uint64_t> &sizes, uint32_t n_up, uint64_t cost) {
    expect(L.n == sizes.size(), what, (long long)L.n, (long long)sizes.size());
    if (L.n != sizes.size()) return;
    uint64_t end = 0, sum = 0;
    for (uint32_t s = 0; s < L.n; ++s) {
        expect(L.off[s] % 16 == 0, "offset is a multiple of 16", s);
        expect(L.off[s] >= end && L.off[s] < end + 16, "sections in order, no overlap, no gap of 16", s);
        expect(L.off[s] + sizes[s] >= L.off[s], "no wrap", s);
        end = L.off[s] + sizes[s];
        sum += sizes[s];
        if (s + 1 == n_up) expect(L.up_bytes == end, "up_bytes ends the last uploaded section", s);
    }
    expect(L.total == end, "total ends the last section");
    expect(sum <= cost, "the sections are inside what the items cost", (long long)sum, (long long)cost);
    expect(L.total <= cost + 16 * (uint64_t)L.n, "total <= costs + 16 x sections", (long long)L.total, (long long)cost);
    expect(L.up_bytes <= L.total, "the upload is inside the arena");
    char base[1];
    expect(L.at<char>(base, L.n - 1) == base + L.off[L.n - 1], "the accessor adds the section's offset");
}

static HbBatchSizes some_sizes() {
    HbBatchSizes z;
    const uint64_t nl = 8ull << (rnd() % 4);   // 8, 16, 32, 64 limbs
    z.limbs = nl * 4;
    z.prf2 = 16 * 15 + 64 + 8 * 2 + 4 * (rnd() % 4);
    z.prf = 16 * 15 + 64 + 4 * nl + 8 + 4 * (rnd() % 4);
    z.file = 40 + 4 * (rnd() % 3);
    z.wg = 8;
    z.vproof = 16;
    z.pproof = 48;
    z.item = 24;
    z.cfile = 48 + 4 * (rnd() % 3);
    return z;
}

static void layouts() {
    for (int round = 0; round < 400; ++round) {
        const HbBatchSizes z = some_sizes();
        const bool big = round % 4 == 3, cxx = round & 1, data_host = round & 2, tags_host = round & 4;
        const uint64_t n = rnd() % 41, S = 1 + rnd() % (big ? 40 : 300), tw = z.limbs - rnd() % 4;
        const uint64_t bpw = 1 + rnd() % 8;
        {   // hb_encode_many / hb_cxx_encode_many
            uint64_t cost = 0, nj = 0, nwg = 0, dbytes = 0, blocks = 0, tbytes = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t len = some_size(big), C = (z.limbs - 1) * S, nb = len / C + 1;
                const uint64_t mb = cxx ? len / C + (len % C ? 1 : 0) : nb;
                const uint64_t j = cxx ? (nb + HB_CB_JOB - 1) / HB_CB_JOB + (S + HB_CB_JOB - 1) / HB_CB_JOB : (S + 15) / 16 + (nb + 15) / 16;
                const uint64_t w = (mb + bpw - 1) / bpw, du = data_host ? hb_up16(len) : 0, tu = tags_host ? hb_up16(nb * tw) : 0;
                cost += hb_enc_cost(z, j, w, du, nb, S, tu);
                nj += j, nwg += w, dbytes += du, blocks += nb, tbytes += tu;
            }
            const HbArena L = hb_enc_arena(z, n, nj, nwg, dbytes, blocks, S, tbytes);
            check_arena("encode", L, {2 * n * z.prf, n * z.file, nj * 16, nwg * z.wg, dbytes, blocks * z.limbs, n * S * z.limbs, tbytes},
                        5, cost);
            expect(L.off[HB_ENC_PRF] == 0 && L.off[HB_ENC_FV] == hb_up16(L.up_bytes) && L.total - L.off[HB_ENC_TAGS] == tbytes,
                   "encode: the named sections");
        }
        {   // hb_verify_rhs_many / hb_cxx_verify_rhs_many
            uint64_t cost = 0, nj = 0, terms = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t c = some_size(big);
                const uint64_t j = cxx ? 2 * ((c + HB_CB_JOB - 1) / HB_CB_JOB) + (S + HB_CB_JOB - 1) / HB_CB_JOB : (S + 15) / 16 + 2 * ((c + 15) / 16);
                cost += hb_verify_cost(z, cxx, j, c, S);
                nj += j, terms += c;
            }
            const HbArena L = hb_verify_arena(z, cxx, n, nj, terms, S);
            check_arena("verify", L, {n * z.prf2, 3 * n * z.prf, cxx ? n * z.item : 0, n * z.vproof, nj * 16, n * S * z.limbs,
                                      terms * z.limbs, terms * z.limbs, n * S * z.limbs, n * z.limbs},
                        6, cost);
            expect(L.off[HB_VER_VV] == hb_up16(L.up_bytes) && L.total - L.off[HB_VER_RES] == n * z.limbs, "verify: the named sections");
            if (!cxx) expect(L.off[HB_VER_ITEMS] == L.off[HB_VER_PROOFS], "verify: the empty section takes no room");
        }
        {   // hb_prove_many / hb_cxx_prove_many
            uint64_t cost = 0, nj = 0, terms = 0, up = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t c = 1 + some_size(big), len = some_size(big), ntags = 1 + some_size(false);
                const uint64_t j = cxx ? 2 * ((c + HB_CB_JOB - 1) / HB_CB_JOB) : 2 * ((c + 15) / 16);
                const uint64_t u = (data_host ? hb_up16(len) : 0) + (tags_host ? hb_up16(ntags * tw) : 0);
                cost += hb_prove_cost(z, cxx, j, c, S, u);
                nj += j, terms += c, up += u;
            }
            const HbArena L = hb_prove_arena(z, cxx, n, nj, up, terms, S);
            check_arena("prove", L, {n * z.prf2, n * z.prf, cxx ? n * z.item : 0, n * (cxx ? z.cfile : z.pproof), nj * 16, up,
                                     terms * 8, terms * z.limbs, n * (S + 1) * z.limbs, cxx ? n * 4 : 0},
                        6, cost);
            expect(L.off[HB_PRV_DATA] + up == L.up_bytes && L.off[HB_PRV_IDX] == hb_up16(L.up_bytes), "prove: the named sections");
            // results and status words come back in one copy
            expect(L.off[HB_PRV_STATUS] == L.off[HB_PRV_RES] + n * (S + 1) * z.limbs, "prove: status follows the results");
            expect(L.total - L.off[HB_PRV_RES] == n * (S + 1) * z.limbs + (cxx ? n * 4 : 0), "prove: the download");
        }
    }
    {   // a group at the byte cap: no wrap, and the bound still holds
        const HbBatchSizes z = some_sizes();
        const uint64_t S = 10, n = HB_BATCH_BYTES / z.limbs / 2;
        const uint64_t j = (S + 15) / 16 + 2 * ((n + 15) / 16), cost = hb_verify_cost(z, false, j, n, S);
        expect(cost >= HB_BATCH_BYTES && cost < 2 * HB_BATCH_BYTES, "one item at the cap", (long long)cost);
        const HbArena L = hb_verify_arena(z, false, 1, j, n, S);
        expect(L.total <= cost + 16 * (uint64_t)L.n && L.total >= cost, "total at the cap", (long long)L.total, (long long)cost);
        const HbArena E = hb_enc_arena(z, 1, 1, 1, HB_BATCH_BYTES, 1, S, 16);
        expect(E.up_bytes > HB_BATCH_BYTES && E.total > E.up_bytes && E.total < 2 * HB_BATCH_BYTES, "a file of the cap's size");
    }
}

// ------------------------------------------------------------------ grouping
struct Greedy {
    std::vector<std::vector<uint64_t>> groups;
    std::vector<uint64_t> rest;
};

// The loop of verify_many_impl before the shared grouping, transcribed:
// batched(i) is units <= bound (its callers' bound never exceeds cap_units),
// `terms` its units, cost_of(i) its bytes.
static Greedy greedy(const std::vector<HbCbItemReq> &it, uint64_t bound, uint64_t cap_chunks, uint64_t cap_bytes) {
    Greedy R;
    std::vector<uint64_t> g;
    const uint64_t nproofs = it.size();
    for (uint64_t i = 0; i < nproofs;) {
        g.clear();
        uint64_t terms = 0, bytes = 0;
        for (; i < nproofs; ++i) {
            if (!(it[i].units <= bound)) {
                R.rest.push_back(i);
                continue;
            }
            const uint64_t n = it[i].units, cost = it[i].bytes;
            if (!g.empty() && (n > cap_chunks - terms || bytes + cost > cap_bytes)) break;
            g.push_back(i);
            terms += n;
            bytes += cost;
        }
        if (!g.empty()) R.groups.push_back(g);
    }
    return R;
}

static void same_groups(const char *what, const std::vector<HbCbItemReq> &it, uint64_t bound, uint64_t cap_units, uint64_t cap_bytes) {
    const Greedy W = greedy(it, bound, cap_units, cap_bytes);
    const HbCbPlan P = hb_batch_groups(it.data(), it.size(), bound, cap_units, cap_bytes);
    expect(P.through == W.rest, what);
    expect(P.groups.size() == W.groups.size(), what, (long long)P.groups.size(), (long long)W.groups.size());
    expect(P.jobs.empty(), "the grouping builds no wave-jobs");
    if (P.groups.size() != W.groups.size()) return;
    uint64_t at = 0;
    for (size_t k = 0; k < P.groups.size(); ++k) {
        const HbCbGroup &G = P.groups[k];
        expect(G.item0 == at && G.nitems == W.groups[k].size(), "the same groups", (long long)k);
        if (G.item0 != at || G.nitems != W.groups[k].size()) return;
        uint64_t units = 0, bytes = 0;
        for (uint64_t f = 0; f < G.nitems; ++f) {
            expect(P.order[at + f] == W.groups[k][f], "the same items in the same order");
            expect(P.ubase[at + f] == units, "ubase is the running sum");
            units += it[W.groups[k][f]].units;
            bytes += it[W.groups[k][f]].bytes;
        }
        expect(G.units == units && G.bytes == bytes && G.job0 == 0 && G.njobs == 0, "group totals");
        at += G.nitems;
    }
    expect(at == P.order.size() && P.order.size() == P.ubase.size(), "the groups cover the order");
    // and hb_cbatch_plan is the grouping plus the wave-job queues
    const HbCbPlan Q = hb_cbatch_plan(it.data(), it.size(), bound, cap_units, cap_bytes);
    expect(Q.order == P.order && Q.ubase == P.ubase && Q.through == P.through && Q.groups.size() == P.groups.size(),
           "hb_cbatch_plan groups alike");
}

static void grouping() {
    auto item = [](uint64_t units, uint64_t bytes) {
        HbCbItemReq R = {};
        R.units = units;
        R.bytes = bytes;
        R.n[HB_CB_V] = units < 1000 ? units : 0;
        R.aes[HB_CB_V] = 1;
        return R;
    };
    same_groups("no items", {}, 10, 10, 10);
    same_groups("items without units", {item(0, 5), item(0, 5), item(0, 5)}, 4, 4, 10);
    same_groups("all above the bound", {item(5, 1), item(~0ull, 1), item(6, 1)}, 4, 9, 100);
    same_groups("one item alone above the byte cap", {item(1, 400), item(1, 5000), item(1, 300), item(1, 700), item(1, 1)}, 9, 9, 1000);
    same_groups("one item alone fills the unit cap", {item(3, 1), item(7, 1), item(1, 1), item(7, 1), item(7, 1)}, 7, 7, 100);
    same_groups("caps of 1", {item(1, 1), item(0, 1), item(1, 1), item(2, 1), item(1, 0), item(0, 0)}, 1, 1, 1);
    same_groups("the bound below the cap", {item(3, 1), item(4, 1), item(5, 1), item(2, 1), item(2, 1)}, 4, 6, 100);
    for (int round = 0; round < 300; ++round) {
        std::vector<HbCbItemReq> it;
        const uint64_t cap_units = 1 + rnd() % (round % 3 ? 60 : 3), bound = 1 + rnd() % cap_units;
        const uint64_t cap_bytes = 1 + rnd() % (round % 5 ? 3000 : 2);
        const uint64_t n = rnd() % 60;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t k = rnd() % 12;
            const uint64_t units = k == 0 ? 0 : k == 1 ? ~0ull : k == 2 ? bound : k == 3 ? bound + 1 : rnd() % (bound + 2);
            const uint64_t bytes = k == 4 ? cap_bytes + 1 + rnd() % 50 : k == 5 ? cap_bytes : k == 6 ? 0 : rnd() % (cap_bytes + 1);
            it.push_back(item(units, bytes));
        }
        same_groups("random", it, bound, cap_units, cap_bytes);
    }
}

// ------------------------------------------------------------------ conversions
static void conversions() {
    const size_t tws[] = {1, 3, 4, 5, 31, 32, 33, 128, 256};
    for (size_t tw : tws)
        for (int round = 0; round < 20; ++round) {
            const size_t nl = (tw + 3) / 4 + (size_t)(round % 3);   // upper limbs to fill with zeros
            std::vector<uint8_t> be(tw), back(tw, 0xaa);
            for (uint8_t &b : be) b = (uint8_t)rnd();
            if (round == 0) memset(be.data(), 0xff, tw);
            std::vector<uint32_t> limbs(nl, 0xdeadbeefu), hand(nl, 0xdeadbeefu);
            hbhost::be_to_limbs(be.data(), tw, limbs.data(), nl);
            // the hand loop of the verify paths, transcribed (o: nl limbs, src: tw bytes)
            {
                uint32_t *o = hand.data();
                const uint8_t *src = be.data();
                memset(o, 0, nl * 4);
                for (uint32_t b = 0; b < tw; ++b) o[b / 4] |= (uint32_t)src[tw - 1 - b] << (8 * (b % 4));
            }
            expect(limbs == hand, "be_to_limbs is the hand loop", (long long)tw, (long long)nl);
            for (size_t t = (tw + 3) / 4; t < nl; ++t) expect(limbs[t] == 0, "upper limbs are zero", (long long)t);
            hbhost::to_be(limbs.data(), nl, back.data(), tw);
            expect(back == be, "be_to_limbs then to_be is the identity", (long long)tw);
            // the results' hand loop, transcribed, is to_be
            std::vector<uint8_t> out(tw, 0x55);
            for (uint32_t b = 0; b < tw; ++b) out[tw - 1 - b] = (uint8_t)(limbs[b / 4] >> (8 * (b % 4)));
            expect(out == back, "to_be is the results' hand loop", (long long)tw);
        }
    {   // more bytes than limbs: the excess is dropped, nothing is written past dst
        const uint8_t be[6] = {1, 2, 3, 4, 5, 6};
        uint32_t one[1] = {0};
        hbhost::be_to_limbs(be, 6, one, 1);
        expect(one[0] == 0x03040506u, "the low limb of a wider value", one[0]);
    }
}

static void switches() {
    expect(hb_test_cap(nullptr) == ~0ull, "no switch: no cap");
    expect(hb_test_cap("0") == 1 && hb_test_cap("junk") == 1, "at least 1");
    expect(hb_test_cap("1") == 1 && hb_test_cap("37") == 37, "the switch's value");
    expect(hb_up16(0) == 0 && hb_up16(1) == 16 && hb_up16(16) == 16 && hb_up16(17) == 32, "hb_up16");
}

int main() {
    layouts();
    grouping();
    conversions();
    switches();
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
