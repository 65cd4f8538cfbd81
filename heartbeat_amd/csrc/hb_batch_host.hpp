// hb_batch_host.hpp -- what the six batched calls (hb_encode_many,
// hb_verify_rhs_many, hb_prove_many and their hb_cxx_* twins) decide on the
// host before any HIP call: a group's arena layout and what one item costs in
// it, the grouping itself (hb_cbatch_plan.hpp), the limb conversions of the
// results, and the test switches' caps.  Pure host code: no HIP, no context,
// nothing beyond the standard library and hb_bignum_host.hpp, so that a
// stand-alone program can walk it (tests/batch_host/host_main.cpp, built with
// AddressSanitizer and UBSan).
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "hb_bignum_host.hpp"
#include "hb_cbatch_plan.hpp"

// A group's scratch ends here (a single item may pass it: hb_batch_groups).
#define HB_BATCH_BYTES (1ull << 30)

inline uint64_t hb_up16(uint64_t x) { return (x + 15) & ~15ull; }

// "Cap from a test switch, at least 1": $HB_TEST_BATCH_BLOCKS and
// $HB_TEST_BATCH_CHUNKS.  v: the switch's value, or NULL when it is not set.
inline uint64_t hb_test_cap(const char *v) {
    if (!v) return ~0ull;
    const uint64_t cap = strtoull(v, nullptr, 10);
    return cap < 1 ? 1 : cap;
}

// ------------------------------------------------------------------ arena layout
// One group's device scratch and the pinned staging buffer that mirrors its
// head.  Sections are appended in order, each starting at the next multiple
// of 16: first the uploaded ones, then end_upload(), then the device-only and
// downloaded ones.  A section of no bytes takes no room.
struct HbArena {
    enum { kMaxSections = 16 };
    uint64_t off[kMaxSections];
    uint32_t n = 0;
    uint64_t up_bytes = 0;   // [0, up_bytes): one H2D copy
    uint64_t total = 0;

    uint32_t add(uint64_t bytes) {
        assert(n < kMaxSections);
        off[n] = hb_up16(total);
        total = off[n] + bytes;
        return n++;
    }
    void end_upload() { up_bytes = total; }
    // section s of the arena (or of its staging mirror) at `base`
    template <class T>
    T *at(void *base, uint32_t s) const {
        return (T *)((uint8_t *)base + off[s]);
    }
};

// sizeof of what the sections hold (hb_args.hpp and the *_args.hpp headers;
// the runtime fills this in per limb count, the test program with any sizes)
struct HbBatchSizes {
    uint64_t prf2, prf;     // PrfParams<2>, PrfParams<NL>
    uint64_t limbs;         // NL * 4
    uint64_t file, wg;      // BatchFile, BatchMacWg
    uint64_t vproof;        // VbProof
    uint64_t pproof;        // PbProof
    uint64_t item, cfile;   // CpvItem, CpvFile
};
#define HB_JOB_BYTES 16u    // a wave-job, any call's: four dwords

// hb_encode_many and hb_cxx_encode_many:
//     [prf | files | jobs | wgs | host files] (uploaded) [F | alpha | tags]
// nf files of `blocks` blocks in all, nj wave-jobs, nwg MAC workgroups, dbytes /
// tbytes of host-resident files / host-bound tags (each file's rounded up to 16).
enum { HB_ENC_PRF, HB_ENC_FILES, HB_ENC_JOBS, HB_ENC_WGS, HB_ENC_DATA, HB_ENC_FV, HB_ENC_AM, HB_ENC_TAGS };
inline HbArena hb_enc_arena(const HbBatchSizes &z, uint64_t nf, uint64_t nj, uint64_t nwg, uint64_t dbytes,
                            uint64_t blocks, uint64_t S, uint64_t tbytes) {
    HbArena L;
    L.add(2 * nf * z.prf);
    L.add(nf * z.file);
    L.add(nj * HB_JOB_BYTES);
    L.add(nwg * z.wg);
    L.add(dbytes);
    L.end_upload();
    L.add(blocks * z.limbs);
    L.add(nf * S * z.limbs);
    L.add(tbytes);
    return L;
}
// scratch bytes of one file of nb blocks inside a group (no slack: the byte
// cap decides the groups, the groups the launch counts)
inline uint64_t hb_enc_cost(const HbBatchSizes &z, uint64_t nj, uint64_t nwg, uint64_t data_up, uint64_t nb, uint64_t S,
                            uint64_t tags_up) {
    return 2 * z.prf + z.file + nj * HB_JOB_BYTES + nwg * z.wg + data_up + nb * z.limbs + S * z.limbs + tags_up;
}

// hb_verify_rhs_many:
//     [index schedules | F, v, alpha schedules | proofs | wave-jobs | mu] (uploaded) [v | F | alpha | results]
// hb_cxx_verify_rhs_many (cxx):
//     [index schedules | v, F, alpha schedules | items | proofs | wave-jobs | mu] (uploaded)
//     [v | F | alpha | results]
// np proofs of `terms` (effective) challenge indices in all, nj wave-jobs.
enum { HB_VER_PIDX, HB_VER_PRF, HB_VER_ITEMS, HB_VER_PROOFS, HB_VER_JOBS, HB_VER_MU, HB_VER_VV, HB_VER_FV, HB_VER_AV, HB_VER_RES };
inline HbArena hb_verify_arena(const HbBatchSizes &z, bool cxx, uint64_t np, uint64_t nj, uint64_t terms, uint64_t S) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(3 * np * z.prf);
    L.add(cxx ? np * z.item : 0);
    L.add(np * z.vproof);
    L.add(nj * HB_JOB_BYTES);
    L.add(np * S * z.limbs);
    L.end_upload();
    L.add(terms * z.limbs);
    L.add(terms * z.limbs);
    L.add(np * S * z.limbs);
    L.add(np * z.limbs);
    return L;
}
// scratch bytes of one proof of n (effective) challenge indices and nj wave-jobs
inline uint64_t hb_verify_cost(const HbBatchSizes &z, bool cxx, uint64_t nj, uint64_t n, uint64_t S) {
    const uint64_t cost = z.prf2 + 3 * z.prf + z.vproof + nj * HB_JOB_BYTES + (2 * n + 2 * S + 1) * z.limbs;
    return cxx ? cost + z.item + 64 : cost;
}

// hb_prove_many:
//     [index schedules | v schedules | proofs | wave-jobs | host files and tags] (uploaded) [idx | v | results]
// hb_cxx_prove_many (cxx):
//     [index schedules | v schedules | items | files | wave-jobs | host files and tags] (uploaded)
//     [idx | v | results | status]
// np proofs of `terms` (effective) challenge indices in all, nj wave-jobs,
// up_files bytes of host-resident files and tags (each rounded up to 16).
// HB_PRV_RECS: the proofs (PbProof), cxx: the files (CpvFile).  Results and
// status words are adjacent: one D2H copy of [off[HB_PRV_RES], total).
enum { HB_PRV_PIDX, HB_PRV_PV, HB_PRV_ITEMS, HB_PRV_RECS, HB_PRV_JOBS, HB_PRV_DATA, HB_PRV_IDX, HB_PRV_VV, HB_PRV_RES, HB_PRV_STATUS };
inline HbArena hb_prove_arena(const HbBatchSizes &z, bool cxx, uint64_t np, uint64_t nj, uint64_t up_files, uint64_t terms,
                              uint64_t S) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(np * z.prf);
    L.add(cxx ? np * z.item : 0);
    L.add(np * (cxx ? z.cfile : z.pproof));
    L.add(nj * HB_JOB_BYTES);
    L.add(up_files);
    L.end_upload();
    L.add(terms * 8);
    L.add(terms * z.limbs);
    L.add(np * (S + 1) * z.limbs);
    L.add(cxx ? np * 4 : 0);
    return L;
}
// scratch bytes of one proof of n (effective) challenge indices and nj
// wave-jobs, up_files bytes of which travel in the staging copy
inline uint64_t hb_prove_cost(const HbBatchSizes &z, bool cxx, uint64_t nj, uint64_t n, uint64_t S, uint64_t up_files) {
    const uint64_t cost = z.prf2 + z.prf + nj * HB_JOB_BYTES + n * (8 + z.limbs) + (S + 1) * z.limbs + up_files;
    return cxx ? cost + z.item + z.cfile + 4 + 128 : cost + z.pproof + 64;
}

// ------------------------------------------------------------------ limb conversions
namespace hbhost {

// nbytes big-endian bytes -> nl little-endian limbs (the upper ones zero);
// to_be (hb_bignum_host.hpp) is the way back
inline void be_to_limbs(const uint8_t *src, size_t nbytes, uint32_t *dst, size_t nl) {
    for (size_t t = 0; t < nl; ++t) dst[t] = 0;
    for (size_t b = 0; b < nbytes && b / 4 < nl; ++b) dst[b / 4] |= (uint32_t)src[nbytes - 1 - b] << (8 * (b % 4));
}

}  // namespace hbhost
