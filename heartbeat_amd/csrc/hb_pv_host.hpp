// hb_pv_host.hpp -- what the eight batched prove and verify calls
// (hb_prove_many, hb_verify_rhs_many, hb_prove_mixed, hb_verify_rhs_mixed and
// their hb_cxx_* twins) write into a group's staging buffer, each piece once:
// key schedules under their range templates, host-resident files and tags, the
// load16 decision, mu as limbs, the PySwizzle calls' wave-job queues, and the
// results' way back.  Plans, arena layouts, record types and kernels stay with
// the calls (hb_runtime.cpp); they come here with raw base and table pointers
// and a *view* of their proofs (OneView: a one-prime call's arguments;
// MixedView: a many-owner call's descriptors and prime cache).  Every piece is
// a template over the view, so the one-prime calls keep their constants.
// Pure host code: no HIP, no context; a stand-alone program runs the fills
// over a heap block of a group's exact staging size under ASan and UBSan
// (tests/pv_host/host_main.cpp).  Failure is a status (HbPvStatus).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/hbswizzle.h"
#include "hb_aes_host.hpp"
#include "hb_cpv_args.hpp"
#include "hb_mixed_args.hpp"   // and with it hb_args.hpp, hb_pbatch_args.hpp, hb_vbatch_args.hpp
#include "hb_mixed_host.hpp"   // and with it hb_batch_host.hpp, hb_bignum_host.hpp

namespace hbhost {

struct PrimeInfo {
    int bits = 0, nl = 0;
    u32 ss = 0, tw = 0;
};

template <int NL>
bool make_prf(const uint8_t *key, size_t key_len, const uint8_t *range_be, size_t range_len,
              PrfParams<NL> &P, int &nr) {
    AesKey k;
    if (!aes_expand(key, key_len, k)) return false;
    nr = k.nr;
    memset(&P, 0, sizeof P);
    memcpy(P.rk, k.rk, sizeof(u32) * 4 * (size_t)(k.nr + 1));
    aes_round1_zero_consts(k, P.r1z);
    Limbs R = from_be(range_be, range_len, NL);
    for (int t = 0; t < NL; ++t) P.R[t] = R[t];
    int bits = bitlen_be(range_be, range_len);
    P.nb = (u32)(bits + 7) / 8;
    P.topmask = (1u << (bits - 8 * ((int)P.nb - 1))) - 1u;
    return true;
}

// 16 / 24 / 32 key bytes <-> 10 / 12 / 14 rounds (Nr = Nk + 6, 4 Nk bytes)
inline int aes_rounds(size_t key_len) { return key_len == 16 ? 10 : key_len == 24 ? 12 : 14; }
inline size_t aes_key_len(int nr) { return 4 * (size_t)(nr - 6); }

inline u32 byte_count(const uint8_t *be, size_t n) { return (u32)((bitlen_be(be, n) + 7) / 8); }

inline int u64_be(u64 v, uint8_t out[8]) {
    for (int k = 0; k < 8; ++k) out[k] = (uint8_t)(v >> (56 - 8 * k));
    return 0;
}

// A schedule without its key: what stays is the range, its byte count and top
// mask.  r1z (first-try constants of the lane engine, KeyedPRF's) stays zero:
// the quad engine and the cxx prf have none.
template <class P>
void strip(P &p) {
    memset(p.rk, 0, sizeof p.rk);
    memset(p.r1z, 0, sizeof p.r1z);
}

// A table entry: the template's range, byte count and top mask under the key.
template <int NL>
void schedule(const PrfParams<NL> &tmpl, const AesKey &k, PrfParams<NL> &out) {
    out = tmpl;
    memcpy(out.rk, k.rk, sizeof(u32) * 4 * (size_t)(k.nr + 1));
}
template <int NL>
bool schedule(const PrfParams<NL> &tmpl, const uint8_t *key, size_t key_len, int nr, PrfParams<NL> &out) {
    AesKey k;
    if (!aes_expand(key, key_len, k) || k.nr != nr) return false;
    schedule<NL>(tmpl, k, out);
    return true;
}

// A range template, rebuilt only when the range differs from the last item's
// (p always, v_max and state_chunks / ntags usually the same over a group).
template <int NL>
struct RangeCache {
    PrfParams<NL> tmpl;
    std::string range;
    bool have = false;
    bool get(const uint8_t *key, size_t key_len, const uint8_t *range_be, size_t range_len) {
        if (have && range.size() == range_len && memcmp(range.data(), range_be, range_len) == 0) return true;
        int n0 = 0;
        if (!make_prf<NL>(key, key_len, range_be, range_len, tmpl, n0)) return false;
        strip(tmpl);
        range.assign((const char *)range_be, range_len);
        have = true;
        return true;
    }
    bool get(const uint8_t *key, size_t key_len, u64 range) {
        uint8_t be[8];
        u64_be(range, be);
        return get(key, key_len, be, 8);
    }
};

// The 16-wide wave-jobs of n evaluations of item f under one kind (the
// PySwizzle-side calls; the cxx calls' queues: hb_cbatch_jobs).
template <class Job>
void push_jobs16(Job *jobs, u64 &j, u64 f, u32 kind, u64 n) {
    for (u64 b = 0; b < n; b += 16) jobs[j++] = Job{(u32)f, kind, (u32)b, (u32)(n - b < 16 ? n - b : 16)};
}

// A host-resident input of a group (a file, a tag array): its len bytes go
// into the staging copy at the cursor, which moves on by len rounded up to 16;
// the result is where the kernels find them.  Device-resident: the caller's
// pointer.  (len alone decides what is data: the padding up to the next
// input is never read as sector bytes.)
inline const unsigned char *stage_in(bool on_device, const unsigned char *src, u64 len, uint8_t *host, uint8_t *dev,
                                     u64 &cursor) {
    if (on_device) return src;
    if (len) memcpy(host + cursor, src, (size_t)len);
    const unsigned char *at = dev + cursor;
    cursor += hb_up16(len);
    return at;
}

// What the two proves share: where a proof's file and tags are (stage_in), and
// the results' way back.
struct ProveShape {
    u64 C;
    u32 S, tw;
    bool data_dev, tags_dev;
    u64 up_files(const hb_prove_desc &D) const {   // bytes of the proof that travel in the group's staging copy
        return (data_dev ? 0 : hb_up16(D.len)) + (tags_dev ? 0 : hb_up16(D.ntags * tw));
    }
    // host data: only with host tags and a file prove_impl would upload whole
    // (n: effective chunks); and no proof whose own uploads pass the group cap
    bool uploadable(const hb_prove_desc &D, u64 n) const {
        if (!data_dev) {
            const u64 up_max = 2 * n * C > (8ull << 20) ? 2 * n * C : (8ull << 20);
            if (tags_dev || D.len > up_max || D.len > HB_BATCH_BYTES) return false;
        }
        return tags_dev || D.ntags <= HB_BATCH_BYTES / tw;
    }
};

template <int NL>
void prove_results(const ProveShape &E, const u32 *r, const hb_prove_desc &D) {
    for (u32 k = 0; k < E.S; ++k) to_be(r + (size_t)k * NL, NL, D.mu_out + (size_t)k * E.tw, E.tw);
    to_be(r + (size_t)E.S * NL, NL, D.sigma_out, E.tw);
}

struct MixedCall {
    HbPrimeCache primes;
    std::vector<size_t> prime_of;   // per proof: its entry in `primes`
    std::vector<PrimeInfo> pi;      // per proof
};

template <int NL>
void fill_rec(const HbMxPrime &P, const PrimeInfo &pi, u32 S, u64 col0, u64 slot0, MxRec<NL> &R) {
    memset(&R, 0, sizeof R);
    for (int t = 0; t < NL; ++t) {
        R.mod.p[t] = P.p[t];
        R.r2[t] = P.r2[t];
    }
    R.mod.pinv = P.pinv;
    R.mod.inv_scaled = P.inv_scaled;
    R.C = (u64)pi.ss * S;
    R.ss = pi.ss;
    R.S = S;
    R.tw = pi.tw;
    R.col0 = (u32)col0;
    R.slot0 = (u32)slot0;
}

// ------------------------------------------------------------------ views
// Proof i of a call (i: its position in the call): descriptor, geometry, prime
// bytes, key lengths; count() / at(k): the proofs the call plans, in order.
// Desc: hb_prove_desc or hb_verify_desc (a prove has one key length).
template <class Desc>
struct OneView {
    const Desc *proofs;
    u64 nproofs;
    const uint8_t *p_be_;
    size_t p_len_;
    PrimeInfo pi_;
    u32 S_;
    size_t key_len_, chal_key_len_;
    u64 count() const { return nproofs; }
    u64 at(u64 k) const { return k; }
    const Desc &d(u64 i) const { return proofs[i]; }
    const PrimeInfo &pi(u64) const { return pi_; }
    u32 S(u64) const { return S_; }
    const uint8_t *p_be(u64) const { return p_be_; }
    size_t p_len(u64) const { return p_len_; }
    size_t key_len(u64) const { return key_len_; }
    size_t chal_key_len(u64) const { return chal_key_len_; }
};
typedef OneView<hb_prove_desc> ProveOne;
typedef OneView<hb_verify_desc> VerifyOne;

inline size_t mixed_chal_key_len(const hb_prove_mixed_desc &X) { return (size_t)X.key_len; }
inline size_t mixed_chal_key_len(const hb_verify_mixed_desc &X) { return (size_t)X.chal_key_len; }

// Mixed: hb_prove_mixed_desc or hb_verify_mixed_desc; cls: the class's proofs.
template <class Mixed>
struct MixedView {
    const Mixed *descs;
    const std::vector<u64> *cls;
    const MixedCall *MC;
    u64 count() const { return cls->size(); }
    u64 at(u64 k) const { return (*cls)[(size_t)k]; }
    auto d(u64 i) const -> decltype((descs[i].d)) { return descs[i].d; }
    const PrimeInfo &pi(u64 i) const { return MC->pi[(size_t)i]; }
    u32 S(u64 i) const { return (u32)descs[i].sectors; }
    const uint8_t *p_be(u64 i) const { return descs[i].p_be; }
    size_t p_len(u64 i) const { return (size_t)descs[i].p_len; }
    size_t key_len(u64 i) const { return (size_t)descs[i].key_len; }
    size_t chal_key_len(u64 i) const { return mixed_chal_key_len(descs[i]); }
    const HbMxPrime &prime(u64 i) const { return MC->primes.primes[MC->prime_of[(size_t)i]]; }
};
typedef MixedView<hb_prove_mixed_desc> ProveMixed;
typedef MixedView<hb_verify_mixed_desc> VerifyMixed;

template <class View>
ProveShape prove_shape(const View &V, u64 i, u32 flags) {
    return {(u64)V.pi(i).ss * V.S(i), V.S(i), V.pi(i).tw, (flags & HB_DATA_ON_DEVICE) != 0, (flags & HB_TAGS_ON_DEVICE) != 0};
}

// ------------------------------------------------------------------ the pieces
// HB_PV_KEY: a key does not expand (cxx: or has another round count than the
// launch's); HB_PV_ROUNDS: PySwizzle side, a key of another round count
enum HbPvStatus { HB_PV_OK, HB_PV_KEY, HB_PV_ROUNDS };

// A group never holds more challenge indices than `limit` (2^31; 2^32 - 1 for
// the cxx proves, whose offsets are unsigned int) or the test switch's cap.
inline u64 pv_bound(u64 cap_chunks, u64 limit) { return cap_chunks < limit ? cap_chunks : limit; }

// Effective challenge length.  PySwizzle: chunks.  cxx (check_all,
// cxx/shacham_waters_private.cxx:754-755, 822-827): a challenge of at least
// #tags / state_chunks chunks is every block in order.
inline u64 py_prove_chunks(const hb_prove_desc &D) { return D.chunks; }
inline bool cxx_all(const hb_prove_desc &D) { return D.chunks >= D.ntags; }
inline bool cxx_all(const hb_verify_desc &D) { return D.chunks >= D.state_chunks; }
inline u64 cxx_prove_chunks(const hb_prove_desc &D) { return cxx_all(D) ? D.ntags : D.chunks; }
inline u64 cxx_verify_chunks(const hb_verify_desc &D) { return cxx_all(D) ? D.state_chunks : D.chunks; }

// Prove: the proofs with a challenge, in the call's order; the others get zero
// sums and no GPU work, as prove_impl.  eff: py_prove_chunks or cxx_prove_chunks.
template <class View, class Eff>
std::vector<u64> prove_candidates(const View &V, Eff eff) {
    std::vector<u64> cand;
    for (u64 k = 0; k < V.count(); ++k) {
        const u64 i = V.at(k);
        const hb_prove_desc &D = V.d(i);
        if (eff(D)) {
            cand.push_back(i);
            continue;
        }
        memset(D.mu_out, 0, (size_t)V.S(i) * V.pi(i).tw);
        memset(D.sigma_out, 0, V.pi(i).tw);
    }
    return cand;
}

// Prove: the entries of a group's proofs, one entry() per proof in group
// order.  One AES expansion per challenge key (it serves the index and the v
// schedule) under range templates that are rebuilt only when the range differs
// from the last proof's.  The file and the tags: where they are, or their place
// in the staging copy (cursor: first the data section's offset, at the end the
// arena's up_bytes).  o_pidx, o_pv: the schedule tables' offsets in the arena.
template <int NL>
struct ProveFill {
    uint8_t *host, *dev;          // the staging buffer and the arena it mirrors
    PrfParams<2> *hpidx;          // [proof], in the staging buffer
    PrfParams<NL> *hpv;
    u64 cursor;
    int nr;
    bool cxx, data_dev, tags_dev;
    u32 nb_idx = 0, nb_v = 0;     // the longest try of either kind so far (prove_queue)
    RangeCache<2> PI0;
    RangeCache<NL> PV0;
    ProveFill(uint8_t *host_, uint8_t *dev_, u64 o_pidx, u64 o_pv, u64 o_data, int nr_, bool cxx_, const ProveShape &E)
        : host(host_), dev(dev_), hpidx((PrfParams<2> *)(host_ + o_pidx)), hpv((PrfParams<NL> *)(host_ + o_pv)),
          cursor(o_data), nr(nr_), cxx(cxx_), data_dev(E.data_dev), tags_dev(E.tags_dev) {}

    struct Entry {
        const unsigned char *data, *tags;   // device addresses
        bool load16;
    };
    template <class View>
    HbPvStatus entry(const View &V, u64 i, u64 f, Entry &e) {
        const hb_prove_desc &D = V.d(i);
        const PrimeInfo &pi = V.pi(i);
        const size_t kl = V.chal_key_len(i);
        AesKey kc;
        if (!aes_expand(D.chal_key, kl, kc)) return HB_PV_KEY;
        if (kc.nr != nr) return cxx ? HB_PV_KEY : HB_PV_ROUNDS;
        if (!PI0.get(D.chal_key, kl, D.ntags) || !PV0.get(D.chal_key, kl, D.vmax_be, (size_t)D.vmax_len)) return HB_PV_KEY;
        schedule<2>(PI0.tmpl, kc, hpidx[f]);
        schedule<NL>(PV0.tmpl, kc, hpv[f]);
        if (PI0.tmpl.nb > nb_idx) nb_idx = PI0.tmpl.nb;
        if (PV0.tmpl.nb > nb_v) nb_v = PV0.tmpl.nb;
        e.data = stage_in(data_dev, D.data, D.len, host, dev, cursor);
        e.tags = stage_in(tags_dev, D.tags, D.ntags * pi.tw, host, dev, cursor);
        // per proof, with THIS proof's ss, tw and C
        const bool load16 = pi.ss == 4u * NL && pi.tw == 4u * NL && ((u64)pi.ss * V.S(i)) % 16 == 0 &&
                            (uintptr_t)e.data % 16 == 0 && (uintptr_t)e.tags % 16 == 0;
        e.load16 = load16;
        return HB_PV_OK;
    }
};

// Verify: the entries of a group's proofs.  One AES expansion per key (the
// challenge key's serves the index and the v schedule); the three NL-wide
// schedules of proof f at hprf[3 f + slot], the slots the PySwizzle kernels'
// (HB_VB_*) or the cxx kernels' (HB_CPV_P*); mu as limbs at hmu + mu_base NL.
template <int NL>
struct VerifyFill {
    PrfParams<2> *hpidx;          // [proof], in the staging buffer
    PrfParams<NL> *hprf;          // [3 proof + slot]
    u32 *hmu;
    int nr;
    bool cxx;
    u32 slot_f, slot_v, slot_a;
    const PrfParams<NL> *P0;      // the call's template under p, or NULL: a template per prime (PP0)
    RangeCache<2> PI0;
    RangeCache<NL> PV0, PP0;
    VerifyFill(uint8_t *host, u64 o_pidx, u64 o_prf, u64 o_mu, int nr_, bool cxx_, const PrfParams<NL> *P0_)
        : hpidx((PrfParams<2> *)(host + o_pidx)), hprf((PrfParams<NL> *)(host + o_prf)), hmu((u32 *)(host + o_mu)), nr(nr_),
          cxx(cxx_), slot_f(cxx_ ? HB_CPV_PF : HB_VB_IDXF), slot_v(cxx_ ? HB_CPV_PV : HB_VB_V),
          slot_a(cxx_ ? HB_CPV_PA : HB_VB_ALPHA), P0(P0_) {}

    // n: the proof's effective chunks (chunks, or cxx_verify_chunks)
    template <class View>
    HbPvStatus entry(const View &V, u64 i, u64 f, u64 n, u64 mu_base) {
        const hb_verify_desc &D = V.d(i);
        const PrimeInfo &pi = V.pi(i);
        const size_t kl = V.key_len(i), cl = V.chal_key_len(i);
        const u64 nstate = D.state_chunks ? D.state_chunks : 1;   // (no index is drawn when chunks == 0)
        // v_max is only read when chunks > 0 (the single calls accept any with
        // chunks == 0): one byte for PySwizzle, a 16-byte block for the cxx prf
        static const uint8_t one[16] = {1};
        const uint8_t *vm = n ? D.vmax_be : one;
        const size_t vl = n ? (size_t)D.vmax_len : cxx ? sizeof one : 1;
        AesKey kf, ka, kc;
        if (!aes_expand(D.f_key, kl, kf) || !aes_expand(D.alpha_key, kl, ka) || !aes_expand(D.chal_key, cl, kc))
            return HB_PV_KEY;
        if (kf.nr != nr || ka.nr != nr || kc.nr != nr) return cxx ? HB_PV_KEY : HB_PV_ROUNDS;
        if (!PI0.get(D.chal_key, cl, nstate) || !PV0.get(D.chal_key, cl, vm, vl)) return HB_PV_KEY;
        if (!P0 && !PP0.get(D.f_key, kl, V.p_be(i), V.p_len(i))) return HB_PV_KEY;
        const PrfParams<NL> &PP = P0 ? *P0 : PP0.tmpl;
        schedule<2>(PI0.tmpl, kc, hpidx[f]);
        schedule<NL>(PP, kf, hprf[3 * f + slot_f]);
        schedule<NL>(PV0.tmpl, kc, hprf[3 * f + slot_v]);
        schedule<NL>(PP, ka, hprf[3 * f + slot_a]);
        // mu_j: tw big-endian bytes -> NL little-endian limbs
        const u32 S = V.S(i);
        for (u32 j = 0; j < S; ++j) be_to_limbs(D.mu + (size_t)j * pi.tw, pi.tw, hmu + ((size_t)mu_base + j) * NL, NL);
        return HB_PV_OK;
    }
};

// Queue order of the PySwizzle calls, longest wave-job first (hb_pbatch.hpp,
// hb_vbatch.hpp).  Prove: the kind with the longer tries (v at any v_max of at
// least bytes(ntags) bytes) of every proof, then the other kind.  Verify:
// index + F of every proof, then alpha, then v.  Result: wave-jobs written.
inline u64 prove_queue(PbWaveJob *jobs, const PbProof *proofs, u64 np, u32 nb_idx, u32 nb_v) {
    const u32 kind0 = nb_v >= nb_idx ? HB_PB_V : HB_PB_IDX;
    u64 j = 0;
    for (u32 k = 0; k < 2; ++k)
        for (u64 f = 0; f < np; ++f) push_jobs16(jobs, j, f, k == 0 ? kind0 : 1u - kind0, proofs[f].chunks);
    return j;
}
template <class SOf>
u64 verify_queue(VbWaveJob *jobs, const VbProof *proofs, u64 np, SOf S_of) {
    u64 j = 0;
    for (u64 f = 0; f < np; ++f) push_jobs16(jobs, j, f, HB_VB_IDXF, proofs[f].chunks);
    for (u64 f = 0; f < np; ++f) push_jobs16(jobs, j, f, HB_VB_ALPHA, S_of(f));
    for (u64 f = 0; f < np; ++f) push_jobs16(jobs, j, f, HB_VB_V, proofs[f].chunks);
    return j;
}

// Verify: the rhs of the group's proofs (ids[f]: proof f's position in the
// call) back out of the download, NL limbs each.
template <int NL, class View>
void verify_results(const View &V, const u64 *ids, u64 np, const uint8_t *host) {
    for (u64 f = 0; f < np; ++f) to_be((const u32 *)host + f * NL, NL, V.d(ids[f]).rhs_out, V.pi(ids[f]).tw);
}

}  // namespace hbhost
