// Walks hb_digest_plan (heartbeat_amd/csrc/hb_digest_cache.hpp) through the
// cases of the digest-table policy; built with -fsanitize=address,undefined
// and run by tests/test_digest_plan.py.  Exit status 0 and "ok <n>" on success.
#include <stdio.h>
#include <stdint.h>

#include "hb_digest_cache.hpp"

static int g_checks = 0, g_bad = 0;

static void expect(const char *what, const HbDigPlan &P, uint32_t mode, uint64_t alo, uint64_t ahi, uint64_t vlo,
                   uint64_t vhi, bool keep) {
    ++g_checks;
    const bool ok = P.mode == mode && P.alloc.lo == alo && P.alloc.hi == ahi && P.valid.lo == vlo &&
                    P.valid.hi == vhi && (mode != HB_DIG_STORE || P.keep == keep);
    if (!ok) {
        ++g_bad;
        printf("FAIL %s: mode %u alloc [%llu, %llu) valid [%llu, %llu) keep %d\n", what, P.mode,
               (unsigned long long)P.alloc.lo, (unsigned long long)P.alloc.hi, (unsigned long long)P.valid.lo,
               (unsigned long long)P.valid.hi, (int)P.keep);
    }
}

int main() {
    const uint64_t E = HB_DIG_ENTRY, BIG = 1ull << 40, TOP = ~0ull;
    const HbDigRange none = {0, 0}, v = {100, 200};

    // request contained in the valid range: load, nothing changes
    expect("inside", hb_digest_plan(v, 120, 30, BIG), HB_DIG_LOAD, 100, 200, 100, 200, true);
    expect("whole", hb_digest_plan(v, 100, 100, BIG), HB_DIG_LOAD, 100, 200, 100, 200, true);
    expect("load at a small cap", hb_digest_plan(v, 100, 100, E), HB_DIG_LOAD, 100, 200, 100, 200, true);
    // touching: the union, old entries kept
    expect("touch above", hb_digest_plan(v, 200, 50, BIG), HB_DIG_STORE, 100, 250, 100, 250, true);
    expect("touch below", hb_digest_plan(v, 50, 50, BIG), HB_DIG_STORE, 50, 200, 50, 200, true);
    // overlapping
    expect("overlap above", hb_digest_plan(v, 150, 100, BIG), HB_DIG_STORE, 100, 250, 100, 250, true);
    expect("overlap below", hb_digest_plan(v, 10, 100, BIG), HB_DIG_STORE, 10, 200, 10, 200, true);
    expect("covering", hb_digest_plan(v, 0, 5000, BIG), HB_DIG_STORE, 0, 5000, 0, 5000, true);
    // disjoint: the request replaces the range
    expect("disjoint above", hb_digest_plan(v, 201, 10, BIG), HB_DIG_STORE, 201, 211, 201, 211, false);
    expect("disjoint below", hb_digest_plan(v, 0, 99, BIG), HB_DIG_STORE, 0, 99, 0, 99, false);
    // union over the cap but request under it: the request alone
    expect("union too big", hb_digest_plan(v, 150, 100, 120 * E), HB_DIG_STORE, 150, 250, 150, 250, false);
    expect("union just fits", hb_digest_plan(v, 150, 100, 150 * E), HB_DIG_STORE, 100, 250, 100, 250, true);
    expect("union one short", hb_digest_plan(v, 150, 100, 150 * E - 1), HB_DIG_STORE, 150, 250, 150, 250, false);
    // request over the cap: none, the table stays
    expect("over cap", hb_digest_plan(v, 300, 100, 99 * E), HB_DIG_NONE, 100, 200, 100, 200, true);
    expect("over cap by a byte", hb_digest_plan(v, 300, 100, 100 * E - 1), HB_DIG_NONE, 100, 200, 100, 200, true);
    expect("at the cap", hb_digest_plan(v, 300, 100, 100 * E), HB_DIG_STORE, 300, 400, 300, 400, false);
    // cap 0: off, even for a request inside the valid range
    expect("cap 0, inside", hb_digest_plan(v, 120, 30, 0), HB_DIG_NONE, 100, 200, 100, 200, true);
    expect("cap 0", hb_digest_plan(v, 150, 100, 0), HB_DIG_NONE, 100, 200, 100, 200, true);
    expect("cap 0, empty", hb_digest_plan(none, 0, 1, 0), HB_DIG_NONE, 0, 0, 0, 0, true);
    expect("cap below an entry", hb_digest_plan(none, 0, 1, E - 1), HB_DIG_NONE, 0, 0, 0, 0, true);
    // an empty valid range (also one that "touches" the request at 0)
    expect("empty valid", hb_digest_plan(none, 0, 300, BIG), HB_DIG_STORE, 0, 300, 0, 300, false);
    expect("empty valid, high", hb_digest_plan(none, 7, 3, BIG), HB_DIG_STORE, 7, 10, 7, 10, false);
    const HbDigRange e5 = {5, 5};
    expect("empty valid at 5", hb_digest_plan(e5, 5, 10, BIG), HB_DIG_STORE, 5, 15, 5, 15, false);
    expect("empty request", hb_digest_plan(v, 120, 0, BIG), HB_DIG_NONE, 100, 200, 100, 200, true);
    // ranges near 2^64: no overflow
    const HbDigRange hv = {TOP - 100, TOP - 50};
    expect("high inside", hb_digest_plan(hv, TOP - 90, 40, BIG), HB_DIG_LOAD, TOP - 100, TOP - 50, TOP - 100, TOP - 50,
           true);
    expect("high touch", hb_digest_plan(hv, TOP - 50, 50, BIG), HB_DIG_STORE, TOP - 100, TOP, TOP - 100, TOP, true);
    expect("high end past 2^64 - 1", hb_digest_plan(hv, TOP - 50, 51, BIG), HB_DIG_NONE, TOP - 100, TOP - 50,
           TOP - 100, TOP - 50, true);
    expect("wraps", hb_digest_plan(hv, TOP - 10, 100, TOP), HB_DIG_NONE, TOP - 100, TOP - 50, TOP - 100, TOP - 50, true);
    expect("huge request", hb_digest_plan(none, 0, TOP, TOP), HB_DIG_NONE, 0, 0, 0, 0, true);
    expect("huge request, full cap", hb_digest_plan(none, 0, TOP / E, TOP), HB_DIG_STORE, 0, TOP / E, 0, TOP / E, false);
    const HbDigRange wide = {0, TOP};
    expect("wide valid", hb_digest_plan(wide, TOP - 5, 5, E), HB_DIG_LOAD, 0, TOP, 0, TOP, true);
    expect("far apart", hb_digest_plan(v, TOP - 10, 10, BIG), HB_DIG_STORE, TOP - 10, TOP, TOP - 10, TOP, false);
    expect("far below", hb_digest_plan(hv, 0, 10, TOP), HB_DIG_STORE, 0, 10, 0, 10, false);

    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
