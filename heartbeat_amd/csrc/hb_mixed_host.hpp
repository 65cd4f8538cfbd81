// hb_mixed_host.hpp -- what the mixed-owner batches (hb_prove_mixed,
// hb_verify_rhs_mixed) decide on the host before any HIP call, beyond what
// they share with the one-prime batches (hb_batch_host.hpp): the partition of
// a call's proofs into classes, a group's arena layout and a proof's cost with
// the per-proof records and the workgroup tables, the ragged column and slot
// prefix sums, the workgroup tables themselves, and the cache of Montgomery
// constants per distinct prime.  Pure host code: no HIP, no context, so that a
// stand-alone program can walk it (tests/mixed_host/host_main.cpp, built with
// AddressSanitizer and UBSan).  The cxx Swizzle's mixed-owner batches
// (hb_cxx_prove_mixed, hb_cxx_verify_rhs_mixed) share all of it and add their
// two arena layouts and costs below (tests/cxx_mixed_host/host_main.cpp).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "hb_batch_host.hpp"

// ------------------------------------------------------------------ classes
// A kernel is compiled per limb count (NL) and per AES round count (NR), so
// the proofs of one launch share both.  nl: 8 / 16 / 32 / 64 for the prime's
// bit length; nr: 10 / 12 / 14 for a 16 / 24 / 32-byte key.
inline uint32_t hb_mx_limbs(int bits) { return bits <= 256 ? 8u : bits <= 512 ? 16u : bits <= 1024 ? 32u : bits <= 2048 ? 64u : 0u; }
inline uint32_t hb_mx_rounds(uint64_t key_len) { return key_len == 16 ? 10u : key_len == 24 ? 12u : key_len == 32 ? 14u : 0u; }

struct HbMxClass {
    uint32_t nl, nr;
    std::vector<uint64_t> items;   // positions in the call, in the caller's order
};

// Every item in exactly one class; classes in the order of their first item,
// items inside a class in the caller's order (so a one-prime call is planned
// as hb_prove_many plans it).
inline std::vector<HbMxClass> hb_mixed_partition(const uint32_t *nl, const uint32_t *nr, uint64_t n) {
    std::vector<HbMxClass> out;
    for (uint64_t i = 0; i < n; ++i) {
        size_t k = 0;
        while (k < out.size() && (out[k].nl != nl[i] || out[k].nr != nr[i])) ++k;
        if (k == out.size()) out.push_back(HbMxClass{nl[i], nr[i], {}});
        out[k].items.push_back(i);
    }
    return out;
}

// ------------------------------------------------------------------ tables
// The device reads an entry as two dwords (MxWg, hb_mixed_args.hpp).
struct HbMxWg {
    uint32_t proof, a;
};
#define HB_MXWG_BYTES 8u
#define HB_MX_MONT_TERMS 256u     // terms per workgroup of the conversion pass

// first[f] = sum of (S[g] + add) over g < f; the result is the sum over all n
inline uint64_t hb_mixed_prefix(const uint32_t *S, uint64_t n, uint32_t add, std::vector<uint64_t> &first) {
    first.resize((size_t)n);
    uint64_t at = 0;
    for (uint64_t f = 0; f < n; ++f) {
        first[(size_t)f] = at;
        at += (uint64_t)S[f] + add;
    }
    return at;
}

// sum launch of the prove: one workgroup per (proof, column), S_f + 1 columns
inline uint64_t hb_mixed_sum_wgs(const uint32_t *S, uint64_t n, HbMxWg *out) {
    uint64_t w = 0;
    for (uint64_t f = 0; f < n; ++f)
        for (uint32_t j = 0; j <= S[f]; ++j, ++w)
            if (out) out[w] = HbMxWg{(uint32_t)f, j};
    return w;
}

// conversion pass: workgroup = up to HB_MX_MONT_TERMS terms of ONE proof
inline uint64_t hb_mixed_mont_wg_count(uint64_t chunks) { return (chunks + HB_MX_MONT_TERMS - 1) / HB_MX_MONT_TERMS; }
inline uint64_t hb_mixed_mont_wgs(const uint32_t *chunks, uint64_t n, HbMxWg *out) {
    uint64_t w = 0;
    for (uint64_t f = 0; f < n; ++f)
        for (uint32_t a = 0; a < chunks[f]; a += HB_MX_MONT_TERMS, ++w)
            if (out) out[w] = HbMxWg{(uint32_t)f, a};
    return w;
}

// ------------------------------------------------------------------ arena layout
// hb_prove_mixed:
//     [index schedules | v schedules | proofs | records | sum workgroups | conversion workgroups | wave-jobs |
//      host files and tags] (uploaded) [idx | v | results]
// np proofs of `terms` challenge indices and `cols` result columns in all, nj
// wave-jobs, nmwg conversion workgroups; rec: sizeof(MxRec<NL>).
enum { HB_MXP_PIDX, HB_MXP_PV, HB_MXP_PROOFS, HB_MXP_RECS, HB_MXP_SUMWG, HB_MXP_MONTWG, HB_MXP_JOBS, HB_MXP_DATA,
       HB_MXP_IDX, HB_MXP_VV, HB_MXP_RES, HB_MXP_SECTIONS };
inline HbArena hb_mprove_arena(const HbBatchSizes &z, uint64_t rec, uint64_t np, uint64_t nj, uint64_t cols, uint64_t nmwg,
                               uint64_t up_files, uint64_t terms) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(np * z.prf);
    L.add(np * z.pproof);
    L.add(np * rec);
    L.add(cols * HB_MXWG_BYTES);
    L.add(nmwg * HB_MXWG_BYTES);
    L.add(nj * HB_JOB_BYTES);
    L.add(up_files);
    L.end_upload();
    L.add(terms * 8);
    L.add(terms * z.limbs);
    L.add(cols * z.limbs);
    return L;
}
// scratch bytes of one proof of n challenge indices, S sectors and nj wave-jobs
// (no slack; the section padding is the arena's: at most 16 per section)
inline uint64_t hb_mprove_cost(const HbBatchSizes &z, uint64_t rec, uint64_t nj, uint64_t n, uint64_t S, uint64_t up_files) {
    return z.prf2 + z.prf + z.pproof + rec + (S + 1) * HB_MXWG_BYTES + hb_mixed_mont_wg_count(n) * HB_MXWG_BYTES +
           nj * HB_JOB_BYTES + up_files + n * (8 + z.limbs) + (S + 1) * z.limbs;
}

// hb_verify_rhs_mixed:
//     [index schedules | F, v, alpha schedules | proofs | records | wave-jobs | mu] (uploaded) [v | F | alpha | results]
// np proofs of `terms` challenge indices and `slots` alpha / mu slots in all.
enum { HB_MXV_PIDX, HB_MXV_PRF, HB_MXV_PROOFS, HB_MXV_RECS, HB_MXV_JOBS, HB_MXV_MU, HB_MXV_VV, HB_MXV_FV, HB_MXV_AV,
       HB_MXV_RES, HB_MXV_SECTIONS };
inline HbArena hb_mverify_arena(const HbBatchSizes &z, uint64_t rec, uint64_t np, uint64_t nj, uint64_t terms, uint64_t slots) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(3 * np * z.prf);
    L.add(np * z.vproof);
    L.add(np * rec);
    L.add(nj * HB_JOB_BYTES);
    L.add(slots * z.limbs);
    L.end_upload();
    L.add(terms * z.limbs);
    L.add(terms * z.limbs);
    L.add(slots * z.limbs);
    L.add(np * z.limbs);
    return L;
}
inline uint64_t hb_mverify_cost(const HbBatchSizes &z, uint64_t rec, uint64_t nj, uint64_t n, uint64_t S) {
    return z.prf2 + 3 * z.prf + z.vproof + rec + nj * HB_JOB_BYTES + (2 * n + 2 * S + 1) * z.limbs;
}

// hb_cxx_prove_mixed (z.item: CpvItem, the PRF launch's entry; z.pproof:
// PbProof, the conversion pass's and the sum launch's):
//     [index schedules | v schedules | items | proofs | records | sum workgroups | conversion workgroups | wave-jobs |
//      host files and tags] (uploaded) [idx | v | results | status]
// np proofs of `terms` EFFECTIVE challenge indices and `cols` result columns in
// all, nj wave-jobs of HB_CB_JOB evaluations.  Results and status words are
// adjacent: one D2H copy of [off[HB_CMP_RES], total).
enum { HB_CMP_PIDX, HB_CMP_PV, HB_CMP_ITEMS, HB_CMP_PROOFS, HB_CMP_RECS, HB_CMP_SUMWG, HB_CMP_MONTWG, HB_CMP_JOBS,
       HB_CMP_DATA, HB_CMP_IDX, HB_CMP_VV, HB_CMP_RES, HB_CMP_STATUS, HB_CMP_SECTIONS };
inline HbArena hb_cmprove_arena(const HbBatchSizes &z, uint64_t rec, uint64_t np, uint64_t nj, uint64_t cols, uint64_t nmwg,
                                uint64_t up_files, uint64_t terms) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(np * z.prf);
    L.add(np * z.item);
    L.add(np * z.pproof);
    L.add(np * rec);
    L.add(cols * HB_MXWG_BYTES);
    L.add(nmwg * HB_MXWG_BYTES);
    L.add(nj * HB_JOB_BYTES);
    L.add(up_files);
    L.end_upload();
    L.add(terms * 8);
    L.add(terms * z.limbs);
    L.add(cols * z.limbs);
    L.add(np * 4);
    return L;
}
// scratch bytes of one proof of n effective challenge indices, S sectors and nj
// wave-jobs (exact; the section padding is the arena's: at most 16 per section)
inline uint64_t hb_cmprove_cost(const HbBatchSizes &z, uint64_t rec, uint64_t nj, uint64_t n, uint64_t S, uint64_t up_files) {
    return z.prf2 + z.prf + z.item + z.pproof + rec + (S + 1) * HB_MXWG_BYTES + hb_mixed_mont_wg_count(n) * HB_MXWG_BYTES +
           nj * HB_JOB_BYTES + up_files + n * (8 + z.limbs) + (S + 1) * z.limbs + 4;
}

// hb_cxx_verify_rhs_mixed:
//     [index schedules | v, F, alpha schedules | items | proofs | records | wave-jobs | mu] (uploaded)
//     [v | F | alpha | results]
// np proofs of `terms` effective challenge indices and `slots` alpha / mu slots in all.
enum { HB_CMV_PIDX, HB_CMV_PRF, HB_CMV_ITEMS, HB_CMV_PROOFS, HB_CMV_RECS, HB_CMV_JOBS, HB_CMV_MU, HB_CMV_VV, HB_CMV_FV,
       HB_CMV_AV, HB_CMV_RES, HB_CMV_SECTIONS };
inline HbArena hb_cmverify_arena(const HbBatchSizes &z, uint64_t rec, uint64_t np, uint64_t nj, uint64_t terms, uint64_t slots) {
    HbArena L;
    L.add(np * z.prf2);
    L.add(3 * np * z.prf);
    L.add(np * z.item);
    L.add(np * z.vproof);
    L.add(np * rec);
    L.add(nj * HB_JOB_BYTES);
    L.add(slots * z.limbs);
    L.end_upload();
    L.add(terms * z.limbs);
    L.add(terms * z.limbs);
    L.add(slots * z.limbs);
    L.add(np * z.limbs);
    return L;
}
inline uint64_t hb_cmverify_cost(const HbBatchSizes &z, uint64_t rec, uint64_t nj, uint64_t n, uint64_t S) {
    return z.prf2 + 3 * z.prf + z.item + z.vproof + rec + nj * HB_JOB_BYTES + (2 * n + 2 * S + 1) * z.limbs;
}

// wave-jobs of n evaluations of one kind of a cxx batch (hb_cbatch_jobs)
inline uint64_t hb_cm_jobs(uint64_t n) { return (n + HB_CB_JOB - 1) / HB_CB_JOB; }

// ------------------------------------------------------------------ distinct primes
// The Montgomery constants of a prime (R^2 mod p by 64 NL modular doublings,
// -p^-1 mod 2^32, the scaled 1 / p) are computed once per DISTINCT prime of a
// call: owners repeat.  The key is the prime's big-endian bytes without
// leading zeros, so two spellings of one prime are one entry.
struct HbMxPrime {
    hbhost::Limbs p, r2;          // nl limbs each
    uint32_t pinv;
    double inv_scaled;
    uint32_t nl;
};

struct HbPrimeCache {
    std::map<std::string, size_t> index;
    std::vector<HbMxPrime> primes;
    uint64_t misses = 0;

    static std::string key(const uint8_t *p_be, size_t p_len) {
        size_t z = 0;
        while (z < p_len && p_be[z] == 0) ++z;
        return std::string((const char *)p_be + z, p_len - z);
    }
    // the entry of p (odd, > 1, at most 32 nl bits); a reference stays valid
    // until the next get
    size_t get(const uint8_t *p_be, size_t p_len, uint32_t nl) {
        const std::string k = key(p_be, p_len);
        auto it = index.find(k);
        if (it != index.end()) return it->second;
        HbMxPrime P;
        P.p = hbhost::from_be(p_be, p_len, nl);
        P.r2 = hbhost::pow2_mod(64u * nl, P.p);
        P.pinv = hbhost::mont_pinv(P.p[0]);
        P.inv_scaled = hbhost::inv_scaled(P.p);
        P.nl = nl;
        primes.push_back(P);
        ++misses;
        index[k] = primes.size() - 1;
        return primes.size() - 1;
    }
};
