// hb_prime_host.hpp -- host side of hb_prime_search (pure C++, no HIP): how
// many candidates of a window stay below 2^bits, the batches of the base 2
// pre-pass, and which survivor goes to the full-round launch.  tests/primehost
// runs it against a simulated device.
//
// hb_prime_search's result for a start is the SMALLEST candidate that passes
// base 2 and every given base.  The survivors of the sieve are tested in
// ascending order, a batch per round:
//   ps_plan_base2   jobs for the next batch of every unresolved start;
//   ps_select       per start: the earliest survivor of the batch that passed
//                   base 2 becomes the candidate; if none did, the batch is
//                   behind us;
//   ps_plan_full    a job per base for every candidate;
//   ps_apply_full   all passed: resolved; else the search goes on right after
//                   that candidate (what the batch knew about later survivors
//                   is dropped and they are tested again).
// `next` only ever moves past survivors that were tested and failed, so no
// candidate is reported while a smaller survivor is untested.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "hb_bignum_host.hpp"
#include "hb_prime_args.hpp"

namespace hbhost {

// How many k in [0, window) keep start + 2k below 2^bits (start odd, exactly
// `bits` bits, window <= 2^16): min(window, (2^bits - 1 - start) / 2 + 1).
inline uint32_t ps_window_limit(const Limbs &start, uint32_t bits, uint32_t window) {
    // t = 2^bits - 1 - start: the complement of start within `bits` bits
    for (size_t t = start.size(); t-- > 1;) {
        const uint32_t lo = 32u * (uint32_t)t;
        if (lo >= bits) continue;
        const uint32_t mask = bits - lo >= 32u ? 0xffffffffu : (1u << (bits - lo)) - 1u;
        if (~start[t] & mask) return window;   // t >= 2^32 > 2 window
    }
    const uint32_t mask0 = bits >= 32u ? 0xffffffffu : (1u << bits) - 1u;
    const uint64_t n = (uint64_t)((~start[0] & mask0) >> 1) + 1u;
    return n < window ? (uint32_t)n : window;
}

const uint32_t PS_NONE = 0xffffffffu;

struct PsStart {
    const uint16_t *surv = nullptr;   // the sieve's survivors k, ascending
    uint32_t count = 0;
    uint32_t next = 0;                // survivors [0, next) were tested and failed
    uint32_t b0 = 0, bn = 0;          // the base 2 batch in flight: survivors [b0, b0 + bn)
    uint32_t cand = PS_NONE;          // the survivor in the full-round launch
    uint32_t found = PS_NONE;         // done: the survivor that passed everything, or PS_NONE
    bool done = false;
};

// Survivors per start and round: all unresolved starts together fill the
// machine's `capacity` lanes without overshooting it (one each at the least).
inline uint32_t ps_batch_size(uint64_t capacity, uint64_t nactive) {
    if (!nactive) return 0;
    const uint64_t b = capacity / nactive;
    return b < 1 ? 1u : b > 0xffffffffull ? 0xffffffffu : (uint32_t)b;
}

// Resolves the starts whose survivors are used up (nothing found), then
// appends a base 2 job per survivor of every other unresolved start's next
// batch.  Returns the number of starts still active.
inline size_t ps_plan_base2(std::vector<PsStart> &S, uint64_t capacity, std::vector<PrJob> &jobs) {
    jobs.clear();
    size_t nactive = 0;
    for (PsStart &s : S) {
        if (!s.done && s.next >= s.count) s.done = true;
        if (!s.done) ++nactive;
    }
    const uint32_t b = ps_batch_size(capacity, nactive);
    for (size_t i = 0; i < S.size(); ++i) {
        PsStart &s = S[i];
        if (s.done) continue;
        s.b0 = s.next;
        s.bn = s.count - s.next < b ? s.count - s.next : b;
        for (uint32_t j = 0; j < s.bn; ++j) jobs.push_back(PrJob{(uint32_t)i, s.surv[s.b0 + j], 0u});
    }
    return nactive;
}

// pass: the base 2 verdicts in ps_plan_base2's job order
inline void ps_select(std::vector<PsStart> &S, const uint32_t *pass) {
    size_t off = 0;
    for (PsStart &s : S) {
        if (s.done) continue;
        s.cand = PS_NONE;
        for (uint32_t j = 0; j < s.bn; ++j)
            if (pass[off + j]) {
                s.cand = s.b0 + j;
                break;
            }
        if (s.cand == PS_NONE) s.next = s.b0 + s.bn;
        off += s.bn;
    }
}

// a job per base of every candidate; base r of start i is bases[i * rounds + r]
inline void ps_plan_full(const std::vector<PsStart> &S, uint32_t rounds, std::vector<PrJob> &jobs) {
    jobs.clear();
    for (size_t i = 0; i < S.size(); ++i) {
        const PsStart &s = S[i];
        if (s.done || s.cand == PS_NONE) continue;
        for (uint32_t r = 0; r < rounds; ++r)
            jobs.push_back(PrJob{(uint32_t)i, s.surv[s.cand], (uint32_t)(i * rounds + r)});
    }
}

// pass: the verdicts in ps_plan_full's job order (rounds == 0: none needed)
inline void ps_apply_full(std::vector<PsStart> &S, uint32_t rounds, const uint32_t *pass) {
    size_t off = 0;
    for (PsStart &s : S) {
        if (s.done || s.cand == PS_NONE) continue;
        bool all = true;
        for (uint32_t r = 0; r < rounds; ++r) all = all && pass[off + r] != 0;
        off += rounds;
        if (all) {
            s.found = s.cand;
            s.done = true;
        } else {
            s.next = s.cand + 1;
        }
        s.cand = PS_NONE;
    }
}

// the odd primes below 2^16 (6541 of them)
inline std::vector<uint32_t> ps_sieve_primes() {
    std::vector<uint8_t> comp(65536, 0);
    std::vector<uint32_t> q;
    for (uint32_t i = 3; i < 65536u; i += 2) {
        if (comp[i]) continue;
        q.push_back(i);
        for (uint32_t j = i * i; j < 65536u && i < 256u; j += 2 * i) comp[j] = 1;
    }
    return q;
}

}  // namespace hbhost
