// hb_digest_cache.hpp -- policy of the context's table of per-index SHA-256
// digests (hb_runtime.cpp, two-pass encode).  SHA256(str(i)) depends on the
// block index i alone, so a context keeps the digests of one contiguous index
// range [lo, hi) on the device, 32 bytes per index (8 big-endian words), and
// later encodes of indices inside it load them instead of hashing.
// Plain host C++, no HIP: tests/test_digest_plan.py builds it stand-alone.
#pragma once
#include <stdint.h>

// what the encode kernels do with the table (EncodeArgs::dig_mode, wave-uniform)
#define HB_DIG_NONE 0u    // hash every index (no table)
#define HB_DIG_STORE 1u   // hash, and store the digest into the table
#define HB_DIG_LOAD 2u    // read the digest from the table
#define HB_DIG_ENTRY 32u  // bytes per index

struct HbDigRange {
    uint64_t lo, hi;      // [lo, hi); empty when lo == hi
};

struct HbDigPlan {
    uint32_t mode;
    HbDigRange alloc;     // indices the table must hold for this call (entry 0 = alloc.lo)
    HbDigRange valid;     // the valid range once a store-mode call has completed
    bool keep;            // the old valid entries move into the new table
};

// One decision per hb_encode call, for the call's whole index range
// [req_lo, req_lo + req_n).  `valid` is the range the table holds now,
// `cap_bytes` the most the table may take.
//   cap below one entry (0: off)              -> none
//   request inside valid                      -> load
//   valid and request overlap or touch, and
//   their union fits the cap                  -> store into the union (old entries kept)
//   the request alone fits the cap            -> store into a table of the request
//   otherwise                                 -> none (alloc and valid unchanged)
// What the caller (hb_runtime.cpp, dig_prepare) makes of a store: with `keep`
// it allocates the new table beside the old one and copies the valid entries
// over, so both exist for a moment (up to nearly twice the cap of device
// memory); without `keep` the old valid range is dropped before the encode
// runs (the buffer is reused), so an encode that then fails leaves the table
// empty rather than as it was.
static inline HbDigPlan hb_digest_plan(HbDigRange valid, uint64_t req_lo, uint64_t req_n, uint64_t cap_bytes) {
    HbDigPlan P;
    P.mode = HB_DIG_NONE;
    P.alloc = valid;
    P.valid = valid;
    P.keep = true;
    const uint64_t cap = cap_bytes / HB_DIG_ENTRY;       // entries
    if (cap == 0) return P;
    if (req_n == 0 || req_lo + req_n < req_lo) return P; // empty, or past 2^64 - 1
    const uint64_t req_hi = req_lo + req_n;
    const bool have = valid.hi > valid.lo;
    if (have && valid.lo <= req_lo && req_hi <= valid.hi) {
        P.mode = HB_DIG_LOAD;
        return P;
    }
    if (have && req_lo <= valid.hi && valid.lo <= req_hi) {
        const uint64_t lo = valid.lo < req_lo ? valid.lo : req_lo;
        const uint64_t hi = valid.hi > req_hi ? valid.hi : req_hi;
        if (hi - lo <= cap) {
            P.mode = HB_DIG_STORE;
            P.alloc.lo = P.valid.lo = lo;
            P.alloc.hi = P.valid.hi = hi;
            return P;
        }
    }
    if (req_n <= cap) {
        P.mode = HB_DIG_STORE;
        P.alloc.lo = P.valid.lo = req_lo;
        P.alloc.hi = P.valid.hi = req_hi;
        P.keep = false;
    }
    return P;
}
