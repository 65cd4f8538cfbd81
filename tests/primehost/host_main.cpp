// Stand-alone check of heartbeat_amd/csrc/hb_prime_host.hpp (built with
// AddressSanitizer and UBSan by tests/test_prime_host.py): the batch and
// selection logic of hb_prime_search against a simulated device whose base 2
// and full-round verdicts are random tables, the window limit at its edges,
// and the sieve's prime table.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "hb_prime_host.hpp"

using namespace hbhost;

static unsigned long long g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

struct Sim {
    std::vector<uint16_t> surv;
    std::vector<uint8_t> b2;                 // base 2 verdict per survivor
    std::vector<std::vector<uint8_t>> full;  // verdict per survivor and base
    std::vector<uint8_t> t2, tf;             // tested by a base 2 / a full-round job
};

// one search over nstarts simulated starts; p2 / pf: pass rates in 1/256
static void run_case(size_t nstarts, uint32_t maxcount, uint64_t capacity, uint32_t rounds, unsigned p2, unsigned pf) {
    std::vector<Sim> sim(nstarts);
    std::vector<PsStart> S(nstarts);
    for (size_t i = 0; i < nstarts; ++i) {
        Sim &m = sim[i];
        const uint32_t count = maxcount ? (uint32_t)(rnd() % (maxcount + 1)) : 0;
        uint32_t k = (uint32_t)(rnd() % 3);
        for (uint32_t j = 0; j < count; ++j) {
            m.surv.push_back((uint16_t)k);
            k += 1 + (uint32_t)(rnd() % 5);
            m.b2.push_back((rnd() & 255) < p2);
            std::vector<uint8_t> f(rounds);
            for (uint32_t r = 0; r < rounds; ++r) f[r] = (rnd() & 255) < pf;
            m.full.push_back(f);
        }
        m.t2.assign(count, 0);
        m.tf.assign(count, 0);
        S[i].surv = m.surv.data();
        S[i].count = count;
    }
    std::vector<PrJob> jobs;
    std::vector<uint32_t> pass;
    size_t rounds_run = 0;
    for (;;) {
        size_t before_active = 0;
        for (const PsStart &s : S) before_active += !s.done && s.next < s.count;
        const size_t nactive = ps_plan_base2(S, capacity, jobs);
        CHECK(nactive == before_active);
        if (!nactive) {
            CHECK(jobs.empty());
            break;
        }
        // the batch fills the capacity without overshooting it (one per start at the least)
        const uint32_t b = ps_batch_size(capacity, nactive);
        CHECK(b >= 1 && (b == 1 || (uint64_t)b * nactive <= capacity) && ((uint64_t)(b + 1) * nactive > capacity || b == 1));
        CHECK(jobs.size() <= (uint64_t)b * nactive && !jobs.empty());
        pass.assign(jobs.size(), 0);
        size_t at = 0;
        for (size_t i = 0; i < nstarts; ++i) {
            if (S[i].done) continue;
            CHECK(S[i].b0 == S[i].next && S[i].bn >= 1 && S[i].bn <= b && S[i].b0 + S[i].bn <= S[i].count);
            CHECK(S[i].bn == b || S[i].b0 + S[i].bn == S[i].count);
            for (uint32_t j = 0; j < S[i].bn; ++j, ++at) {
                const PrJob &J = jobs[at];
                const uint32_t idx = S[i].b0 + j;
                CHECK(J.src == i && J.k == sim[i].surv[idx]);
                sim[i].t2[idx] = 1;
                pass[at] = sim[i].b2[idx];
            }
        }
        CHECK(at == jobs.size());
        ps_select(S, pass.data());
        ps_plan_full(S, rounds, jobs);
        pass.assign(jobs.size(), 0);
        at = 0;
        for (size_t i = 0; i < nstarts; ++i) {
            if (S[i].done || S[i].cand == PS_NONE) continue;
            const uint32_t idx = S[i].cand;
            CHECK(idx >= S[i].b0 && idx < S[i].b0 + S[i].bn && sim[i].b2[idx]);
            for (uint32_t j = S[i].b0; j < idx; ++j) CHECK(!sim[i].b2[j]);   // the earliest of the batch
            sim[i].tf[idx] = 1;
            for (uint32_t r = 0; r < rounds; ++r, ++at) {
                CHECK(jobs[at].src == i && jobs[at].k == sim[i].surv[idx] && jobs[at].base == i * rounds + r);
                pass[at] = sim[i].full[idx][r];
            }
        }
        CHECK(at == jobs.size());
        ps_apply_full(S, rounds, pass.data());
        CHECK(++rounds_run <= (size_t)maxcount * 2 + 2);   // every round moves every active start on
    }
    for (size_t i = 0; i < nstarts; ++i) {
        const Sim &m = sim[i];
        uint32_t want = PS_NONE;
        for (uint32_t j = 0; j < S[i].count && want == PS_NONE; ++j) {
            bool all = m.b2[j] != 0;
            for (uint32_t r = 0; r < rounds; ++r) all = all && m.full[j][r];
            if (all) want = j;
        }
        CHECK(S[i].done && S[i].found == want);
        // never past an untested smaller survivor
        const uint32_t upto = want == PS_NONE ? S[i].count : want + 1;
        for (uint32_t j = 0; j < upto; ++j) {
            CHECK(m.t2[j]);
            if (m.b2[j]) CHECK(m.tf[j]);
        }
    }
}

static Limbs limbs_of(unsigned __int128 v, size_t nl) {
    Limbs r(nl, 0);
    for (size_t t = 0; t < nl && t < 4; ++t) r[t] = (uint32_t)(v >> (32 * t));
    return r;
}

static void window_cases() {
    // exhaustive against 128-bit arithmetic at small sizes
    for (uint32_t bits : {8u, 9u, 16u, 17u, 31u, 32u, 33u, 63u, 64u}) {
        const unsigned __int128 top = (unsigned __int128)1 << bits;
        for (int rep = 0; rep < 400; ++rep) {
            unsigned __int128 start;
            if (rep < 200 && 2 * (unsigned __int128)rep >= top / 2) continue;      // would leave `bits` bits
            if (rep < 200) start = top - 1 - 2 * (unsigned __int128)rep;           // near 2^bits
            else start = (((unsigned __int128)rnd() % (top / 2)) + top / 2) | 1;  // anywhere
            for (uint32_t window : {1u, 2u, 5u, 64u, 100u, 199u, 200u, 201u, 1024u, 65535u, 65536u}) {
                const unsigned __int128 room = (top - 1 - start) / 2 + 1;
                const uint32_t want = room < window ? (uint32_t)room : window;
                CHECK(ps_window_limit(limbs_of(start, 2), bits, window) == want);
                CHECK(ps_window_limit(limbs_of(start, 8), bits, window) == want);
            }
        }
    }
    // wide starts: all-ones upper limbs decide
    for (uint32_t bits : {65u, 128u, 129u, 1000u, 1024u, 2047u, 2048u}) {
        const size_t nl = bits <= 256 ? 8 : bits <= 512 ? 16 : bits <= 1024 ? 32 : 64;
        Limbs ones(nl, 0);
        for (uint32_t b = 0; b < bits; ++b) ones[b / 32] |= 1u << (b % 32);
        for (uint32_t back : {0u, 1u, 7u, 4095u, 4096u, 65535u, 65536u, 70000u}) {
            Limbs s(ones);
            s[0] -= 2 * back;   // 2^bits - 1 - 2 back (no borrow: back < 2^17)
            for (uint32_t window : {1u, 8u, 4096u, 4097u, 65536u})
                CHECK(ps_window_limit(s, bits, window) == (back + 1 < window ? back + 1 : window));
        }
        Limbs s(ones);
        s[(bits - 2) / 32] &= ~(1u << ((bits - 2) % 32));   // far below 2^bits
        CHECK(ps_window_limit(s, bits, 65536) == 65536);
    }
}

int main() {
    window_cases();
    const std::vector<uint32_t> q = ps_sieve_primes();
    CHECK(q.size() == 6541 && q.front() == 3 && q[1] == 5 && q.back() == 65521);
    for (size_t i = 1; i < q.size(); ++i) CHECK(q[i] > q[i - 1] && (q[i] & 1));
    for (uint32_t v : q)
        for (uint32_t d = 3; d * d <= v && d < 300; d += 2) CHECK(v % d || v == d);
    CHECK(ps_batch_size(100, 0) == 0 && ps_batch_size(0, 3) == 1 && ps_batch_size(65536, 256) == 256);
    // batches of 1, at capacity, capacity + 1 starts, and a roomy machine
    for (int rep = 0; rep < 60; ++rep)
        for (size_t nstarts : {(size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)40})
            for (uint64_t capacity : {(uint64_t)1, (uint64_t)8, (uint64_t)9, (uint64_t)64, (uint64_t)65536})
                for (uint32_t rounds : {0u, 1u, 3u}) {
                    run_case(nstarts, 30, capacity, rounds, 40, 128);    // pseudoprimes common: many restarts
                    run_case(nstarts, 30, capacity, rounds, 20, 255);
                    run_case(nstarts, 12, capacity, rounds, 0, 255);     // nothing passes base 2
                    run_case(nstarts, 5, capacity, rounds, 255, 0);      // everything fails the bases
                    run_case(nstarts, 0, capacity, rounds, 255, 255);    // no survivors at all
                }
    printf("ok %llu\n", g_checks);
    return 0;
}
