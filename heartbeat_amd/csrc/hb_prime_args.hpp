// hb_prime_args.hpp -- argument blocks of the prime kernels (hb_prime.hpp:
// hb_mr_test, hb_prime_search), shared with the host runtime.  Apart from
// hb_args.hpp so that the prime units rebuild alone.
#pragma once
#include <stdint.h>

#define HB_PR_TEST_WG 64u
#define HB_PR_SIEVE_WG 256u
#define HB_PR_MAX_WINDOW 65536u

// One lane's test: is src[src] + 2 k a strong probable prime to bases[base]
// (base 2 launches do not read `base`)?
struct PrJob {
    uint32_t src, k, base;
};

struct PrTestArgs {
    const uint32_t *src;      // numbers, NL little-endian limbs each
    const uint32_t *bases;    // bases, NL limbs each (NULL for a base 2 launch)
    const PrJob *jobs;
    uint32_t *pass;           // pass[j] = 1 or 0
    uint64_t njobs;
    uint32_t maxbits;         // the largest bit length among the launch's candidates
};

struct PrSieveArgs {
    const uint32_t *starts;   // NL limbs per start
    const uint32_t *win;      // per start: candidates start + 2k, k < win, stay below 2^bits
    const uint32_t *q;        // the odd primes below 2^16
    uint32_t nq;
    uint32_t stride;          // survivors of start i at surv[i * stride ..]
    unsigned short *surv;
    uint32_t *count;
};
