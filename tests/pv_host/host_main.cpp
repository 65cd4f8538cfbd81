// The batched prove and verify calls' table fills (heartbeat_amd/csrc/hb_pv_host.hpp)
// against a transcription of the four fill loops they replaced -- prove and
// verify, one prime and many owners, the cxx flavours as a flag -- under
// AddressSanitizer and UBSan.  Both sides fill a heap block of exactly a
// group's staging size (group_arenas: max(up_bytes, total - off[results])), so
// an overrun is a report; compared per case: the whole uploaded range, the
// device addresses of data and tags, every load16 flag, the end cursor against
// up_bytes and the job count against the plan's.  The tables the calls write
// around the pieces (records, workgroup tables, the cxx calls' planned queues)
// are written here as hb_runtime.cpp writes them.
#include <stdio.h>
#include <stdlib.h>

#include "hb_cbatch_args.hpp"
#include "hb_cpv_args.hpp"
#include "hb_cmixed_args.hpp"
#include "hb_pv_host.hpp"

using namespace hbhost;

static long g_checks = 0;
#define CHECK(x)                                                                \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(x)) {                                                             \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #x, g_case); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)
static char g_case[256] = "";

// what the sweep must have reached
static struct {
    long load16_set, load16_clear, range_hit, range_miss, ragged, all_prove, all_verify, no_chunks, vmax_p, vmax_1, dev_odd,
        dev_even;
} g_seen;

// ------------------------------------------------------------------ inputs
struct Prime {
    std::vector<uint8_t> be;
    PrimeInfo pi;
};
static Prime prime_of(int bits, long minus) {   // 2^bits - minus (odd)
    Prime P;
    const size_t n = (size_t)(bits + 8) / 8;
    std::vector<uint8_t> v(n, 0);
    v[n - 1 - (size_t)bits / 8] = (uint8_t)(1u << (bits % 8));
    long borrow = minus;
    for (size_t k = n; k-- > 0 && borrow;) {
        long d = (long)v[k] - (borrow & 0xff);
        borrow >>= 8;
        if (d < 0) {
            d += 256;
            ++borrow;
        }
        v[k] = (uint8_t)d;
    }
    size_t z = 0;
    while (v[z] == 0) ++z;
    P.be.assign(v.begin() + (long)z, v.end());
    P.pi.bits = bitlen_be(P.be.data(), P.be.size());
    P.pi.nl = P.pi.bits <= 256 ? 8 : P.pi.bits <= 512 ? 16 : 32;
    P.pi.ss = (u32)P.pi.bits / 8;
    P.pi.tw = (u32)(P.pi.bits + 7) / 8;
    return P;
}
static Prime p256() {   // 2^256 - 2^224 + 2^192 + 2^96 - 1
    static const uint8_t be[32] = {0xff, 0xff, 0xff, 0xff, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0,
                                   0, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    Prime P;
    P.be.assign(be, be + 32);
    P.pi.bits = 256;
    P.pi.nl = 8;
    P.pi.ss = P.pi.tw = 32;
    return P;
}

static u64 g_rng = 0x9e3779b97f4a7c15ull;
static u32 rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (u32)(g_rng >> 33);
}
static std::vector<uint8_t> bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = (uint8_t)rnd();
    return v;
}

// One proof of a group, prove or verify; the descriptors point into it.
struct Item {
    const Prime *P;
    u32 S;
    u64 chunks, ntags, state_chunks, len;
    std::vector<uint8_t> key, fkey, akey, vmax, data, tags, mu, out;
    const uint8_t *dev_data, *dev_tags;   // what the descriptor names when the input is device-resident
};

template <int NL>
static HbBatchSizes sizes() {
    return {sizeof(PrfParams<2>), sizeof(PrfParams<NL>), NL * 4,         sizeof(BatchFile), sizeof(BatchMacWg),
            sizeof(VbProof),      sizeof(PbProof),       sizeof(CpvItem), sizeof(CpvFile)};
}

// a device arena that is never touched: only its addresses are compared
static uint8_t *const kDev = (uint8_t *)(uintptr_t)0x7f0000000000ull;

struct Out {
    std::vector<const unsigned char *> ddata, dtags;
    std::vector<int> load16;
    u64 cursor = 0, njobs = 0;
    int status = 0;   // 0, 1: "invalid (challenge) key", 2: "internal: AES round counts differ"
};

// ------------------------------------------------------------------ prove
template <int NL>
struct ProveTables {
    uint8_t *host;
    PrfParams<2> *hpidx;
    PrfParams<NL> *hpv;
    CpvItem *hitems;      // cxx
    void *hrecs;          // PbProof, or CpvFile (one prime, cxx)
    MxRec<NL> *hmx;       // many owners
    PbWaveJob *hjobs;     // PySwizzle
    u64 data_off, up_bytes;
};

// hb_runtime.cpp before the shared header: prove_many_impl / cxx_prove_many_impl
template <int NL>
static void ref_prove_one(const ProveTables<NL> &T, bool cxx, const PrimeInfo &pi, u32 S, size_t key_len, bool data_dev,
                          bool tags_dev, const hb_prove_desc *proofs, const u64 *ubase, u64 np, Out &O) {
    const int nr = aes_rounds(key_len);
    const u64 C = (u64)pi.ss * S;
    uint8_t *host = T.host, *dev = kDev;
    u64 o_next = T.data_off;
    u32 nb_idx = 0, nb_v = 0;
    RangeCache<2> PI0;
    RangeCache<NL> PV0;
    for (u64 f = 0; f < np; ++f) {
        const hb_prove_desc &D = proofs[f];
        if (!cxx) {
            if (!PI0.get(D.chal_key, key_len, D.ntags) || !PV0.get(D.chal_key, key_len, D.vmax_be, (size_t)D.vmax_len)) {
                O.status = 1;
                return;
            }
            AesKey kc;
            if (!aes_expand(D.chal_key, key_len, kc)) {
                O.status = 1;
                return;
            }
            if (kc.nr != nr) {
                O.status = 2;
                return;
            }
            schedule<2>(PI0.tmpl, kc, T.hpidx[f]);
            schedule<NL>(PV0.tmpl, kc, T.hpv[f]);
            if (PI0.tmpl.nb > nb_idx) nb_idx = PI0.tmpl.nb;
            if (PV0.tmpl.nb > nb_v) nb_v = PV0.tmpl.nb;
        } else if (!PI0.get(D.chal_key, key_len, D.ntags) || !PV0.get(D.chal_key, key_len, D.vmax_be, (size_t)D.vmax_len) ||
                   !schedule<2>(PI0.tmpl, D.chal_key, key_len, nr, T.hpidx[f]) ||
                   !schedule<NL>(PV0.tmpl, D.chal_key, key_len, nr, T.hpv[f])) {
            O.status = 1;
            return;
        }
        const unsigned char *ddata = stage_in(data_dev, D.data, D.len, host, dev, o_next);
        const unsigned char *dtags = stage_in(tags_dev, D.tags, D.ntags * pi.tw, host, dev, o_next);
        const bool load16 = pi.ss == 4u * NL && pi.tw == 4u * NL && C % 16 == 0 && (uintptr_t)ddata % 16 == 0 &&
                            (uintptr_t)dtags % 16 == 0;
        if (!cxx) {
            ((PbProof *)T.hrecs)[f] = PbProof{ubase[f], ddata, D.len, dtags, D.ntags, (u32)D.chunks, load16 ? HB_PB_LOAD16 : 0u};
        } else {
            const bool all = D.chunks >= D.ntags;
            const u64 eff = all ? D.ntags : D.chunks;
            const u32 fl = all ? HB_CPV_ALL : 0u;
            T.hitems[f] = CpvItem{ubase[f], D.ntags, (u32)eff, fl};
            ((CpvFile *)T.hrecs)[f] = CpvFile{ddata, D.len, dtags, D.ntags, ubase[f], (u32)eff, fl | (load16 ? HB_CPV_LOAD16 : 0u)};
        }
        O.ddata.push_back(ddata);
        O.dtags.push_back(dtags);
        O.load16.push_back(load16);
    }
    if (!cxx) {
        const u32 kind0 = nb_v >= nb_idx ? HB_PB_V : HB_PB_IDX;
        u64 j = 0;
        for (u32 k = 0; k < 2; ++k)
            for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, k == 0 ? kind0 : 1u - kind0, ((PbProof *)T.hrecs)[f].chunks);
        O.njobs = j;
    }
    O.cursor = o_next;
}

// prove_mixed_impl / cxx_prove_mixed_impl
template <int NL>
static void ref_prove_mixed(const ProveTables<NL> &T, bool cxx, const hb_prove_mixed_desc *descs, const MixedCall &MC, int nr,
                            bool data_dev, bool tags_dev, const u64 *ubase, const std::vector<u64> &col0, u64 np, Out &O) {
    const size_t key_len = nr == 10 ? 16 : nr == 12 ? 24 : 32;
    uint8_t *host = T.host, *dev = kDev;
    PbProof *hproofs = (PbProof *)T.hrecs;
    u64 o_next = T.data_off;
    u32 nb_idx = 0, nb_v = 0;
    RangeCache<2> PI0;
    RangeCache<NL> PV0;
    for (u64 f = 0; f < np; ++f) {
        const u64 i = f;
        const hb_prove_desc &D = descs[i].d;
        const PrimeInfo &pi = MC.pi[(size_t)i];
        const u32 S = (u32)descs[i].sectors;
        const u64 C = (u64)pi.ss * S;
        if (!cxx) {
            if (!PI0.get(D.chal_key, key_len, D.ntags) || !PV0.get(D.chal_key, key_len, D.vmax_be, (size_t)D.vmax_len)) {
                O.status = 1;
                return;
            }
            AesKey kc;
            if (!aes_expand(D.chal_key, key_len, kc)) {
                O.status = 1;
                return;
            }
            if (kc.nr != nr) {
                O.status = 2;
                return;
            }
            schedule<2>(PI0.tmpl, kc, T.hpidx[f]);
            schedule<NL>(PV0.tmpl, kc, T.hpv[f]);
            if (PI0.tmpl.nb > nb_idx) nb_idx = PI0.tmpl.nb;
            if (PV0.tmpl.nb > nb_v) nb_v = PV0.tmpl.nb;
        } else if (!PI0.get(D.chal_key, key_len, D.ntags) || !PV0.get(D.chal_key, key_len, D.vmax_be, (size_t)D.vmax_len) ||
                   !schedule<2>(PI0.tmpl, D.chal_key, key_len, nr, T.hpidx[f]) ||
                   !schedule<NL>(PV0.tmpl, D.chal_key, key_len, nr, T.hpv[f])) {
            O.status = 1;
            return;
        }
        const unsigned char *ddata = stage_in(data_dev, D.data, D.len, host, dev, o_next);
        const unsigned char *dtags = stage_in(tags_dev, D.tags, D.ntags * pi.tw, host, dev, o_next);
        const bool load16 = pi.ss == 4u * NL && pi.tw == 4u * NL && C % 16 == 0 && (uintptr_t)ddata % 16 == 0 &&
                            (uintptr_t)dtags % 16 == 0;
        if (!cxx) {
            hproofs[f] = PbProof{ubase[f], ddata, D.len, dtags, D.ntags, (u32)D.chunks, load16 ? HB_PB_LOAD16 : 0u};
        } else {
            const bool all = D.chunks >= D.ntags;
            const u64 eff = all ? D.ntags : D.chunks;
            T.hitems[f] = CpvItem{ubase[f], D.ntags, (u32)eff, all ? HB_CPV_ALL : 0u};
            hproofs[f] = PbProof{ubase[f], ddata, D.len, dtags, D.ntags, (u32)eff,
                                 (load16 ? HB_PB_LOAD16 : 0u) | (all ? HB_CMX_ALL : 0u)};
        }
        fill_rec<NL>(MC.primes.primes[MC.prime_of[(size_t)i]], pi, S, col0[(size_t)f], 0, T.hmx[f]);
        O.ddata.push_back(ddata);
        O.dtags.push_back(dtags);
        O.load16.push_back(load16);
    }
    if (!cxx) {
        const u32 kind0 = nb_v >= nb_idx ? HB_PB_V : HB_PB_IDX;
        u64 j = 0;
        for (u32 k = 0; k < 2; ++k)
            for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, k == 0 ? kind0 : 1u - kind0, hproofs[f].chunks);
        O.njobs = j;
    }
    O.cursor = o_next;
}

// the calls as they are now: the header's pieces, the caller's records
template <int NL, class View>
static void new_prove(const ProveTables<NL> &T, bool cxx, bool mixed, const View &V, int nr, u32 flags, const u64 *ubase, u64 np,
                      Out &O) {
    ProveFill<NL> F(T.host, kDev, (u64)((uint8_t *)T.hpidx - T.host), (u64)((uint8_t *)T.hpv - T.host), T.data_off, nr, cxx,
                    prove_shape(V, 0, flags));
    for (u64 f = 0; f < np; ++f) {
        const hb_prove_desc &D = V.d(f);
        typename ProveFill<NL>::Entry e;
        if (HbPvStatus st = F.entry(V, f, f, e)) {
            O.status = st == HB_PV_ROUNDS ? 2 : 1;
            return;
        }
        const bool all = cxx && cxx_all(D);
        const u64 eff = cxx ? cxx_prove_chunks(D) : D.chunks;
        if (cxx) T.hitems[f] = CpvItem{ubase[f], D.ntags, (u32)eff, all ? HB_CPV_ALL : 0u};
        if (cxx && !mixed)
            ((CpvFile *)T.hrecs)[f] = CpvFile{e.data, D.len, e.tags, D.ntags, ubase[f], (u32)eff,
                                              (all ? HB_CPV_ALL : 0u) | (e.load16 ? HB_CPV_LOAD16 : 0u)};
        else
            ((PbProof *)T.hrecs)[f] = PbProof{ubase[f], e.data, D.len, e.tags, D.ntags, (u32)eff,
                                              (e.load16 ? HB_PB_LOAD16 : 0u) | (all ? HB_CMX_ALL : 0u)};
        O.ddata.push_back(e.data);
        O.dtags.push_back(e.tags);
        O.load16.push_back(e.load16);
    }
    if (!cxx) O.njobs = prove_queue(T.hjobs, (const PbProof *)T.hrecs, np, F.nb_idx, F.nb_v);
    O.cursor = F.cursor;
}
template <int NL>
static void new_prove_recs(const ProveTables<NL> &T, const ProveMixed &V, const std::vector<u64> &col0, u64 np) {
    for (u64 f = 0; f < np; ++f) fill_rec<NL>(V.prime(f), V.pi(f), V.S(f), col0[(size_t)f], 0, T.hmx[f]);
}

// One group of proofs through both sides.
template <int NL>
static void prove_case(std::vector<Item> &items, bool cxx, bool mixed, size_t key_len, bool data_dev, bool tags_dev) {
    const u64 np = items.size();
    const HbBatchSizes z = sizes<NL>();
    const u64 rec = sizeof(MxRec<NL>);
    const int nr = aes_rounds(key_len);
    const u32 flags = (data_dev ? HB_DATA_ON_DEVICE : 0u) | (tags_dev ? HB_TAGS_ON_DEVICE : 0u);
    std::vector<hb_prove_mixed_desc> descs((size_t)np);
    std::vector<hb_prove_desc> plain((size_t)np);
    std::vector<u64> cls((size_t)np), ubase((size_t)np), col0;
    std::vector<u32> Sv((size_t)np), nv((size_t)np);
    std::vector<HbCbItemReq> req((size_t)np);
    MixedCall MC;
    u64 terms = 0, up_files = 0, nj = 0;
    for (u64 f = 0; f < np; ++f) {
        Item &I = items[(size_t)f];
        hb_prove_mixed_desc &X = descs[(size_t)f];
        X.p_be = I.P->be.data();
        X.p_len = I.P->be.size();
        X.sectors = I.S;
        X.key_len = key_len;
        X.d = hb_prove_desc{I.key.data(), I.chunks, I.vmax.data(), I.vmax.size(), tags_dev ? I.dev_tags : I.tags.data(), I.ntags,
                            data_dev ? I.dev_data : (I.len ? I.data.data() : nullptr), I.len, I.out.data(), I.out.data()};
        plain[(size_t)f] = X.d;
        cls[(size_t)f] = f;
        MC.prime_of.push_back(MC.primes.get(X.p_be, (size_t)X.p_len, NL));
        MC.pi.push_back(I.P->pi);
        const u64 eff = cxx ? cxx_prove_chunks(X.d) : X.d.chunks;
        CHECK(eff > 0);
        ubase[(size_t)f] = terms;
        terms += eff;
        Sv[(size_t)f] = I.S;
        nv[(size_t)f] = (u32)eff;
        const ProveShape E = {(u64)I.P->pi.ss * I.S, I.S, I.P->pi.tw, data_dev, tags_dev};
        up_files += E.up_files(X.d);
        if (!cxx) nj += 2 * ((eff + 15) / 16);
        req[(size_t)f].n[HB_CB_V] = eff;
        req[(size_t)f].n[HB_CB_IDX] = cxx_all(X.d) ? 0 : eff;
        req[(size_t)f].aes[HB_CB_V] = (byte_count(X.d.vmax_be, (size_t)X.d.vmax_len) + 15) / 16;
        req[(size_t)f].aes[HB_CB_IDX] = 1;
        req[(size_t)f].units = eff;
        if (cxx && cxx_all(X.d)) ++g_seen.all_prove;
    }
    HbCbPlan plan;
    if (cxx) {
        plan = hb_cbatch_plan(req.data(), np, ~0ull, ~0ull, ~0ull);
        CHECK(plan.groups.size() == 1 && plan.groups[0].nitems == np);
        nj = plan.groups[0].njobs;
    }
    const u64 cols = hb_mixed_prefix(Sv.data(), np, 1, col0);
    const u64 nmwg = hb_mixed_mont_wgs(nv.data(), np, nullptr);
    const HbArena L = !mixed ? hb_prove_arena(z, cxx, np, nj, up_files, terms, items[0].S)
                      : cxx  ? hb_cmprove_arena(z, rec, np, nj, cols, nmwg, up_files, terms)
                             : hb_mprove_arena(z, rec, np, nj, cols, nmwg, up_files, terms);
    const u32 down = !mixed ? (u32)HB_PRV_RES : cxx ? (u32)HB_CMP_RES : (u32)HB_MXP_RES;
    const u64 dbytes = L.total - L.off[down];
    const size_t size = (size_t)(L.up_bytes > dbytes ? L.up_bytes : dbytes);
    Out O[2];
    uint8_t *buf[2];
    for (int side = 0; side < 2; ++side) {
        uint8_t *host = buf[side] = (uint8_t *)malloc(size ? size : 1);
        memset(host, 0xA5, size);
        ProveTables<NL> T = {};
        T.host = host;
        T.up_bytes = L.up_bytes;
        u32 jobs_sec;
        if (!mixed) {
            T.hpidx = L.at<PrfParams<2>>(host, HB_PRV_PIDX);
            T.hpv = L.at<PrfParams<NL>>(host, HB_PRV_PV);
            T.hitems = L.at<CpvItem>(host, HB_PRV_ITEMS);
            T.hrecs = L.at<void>(host, HB_PRV_RECS);
            jobs_sec = HB_PRV_JOBS;
            T.data_off = L.off[HB_PRV_DATA];
        } else if (!cxx) {
            T.hpidx = L.at<PrfParams<2>>(host, HB_MXP_PIDX);
            T.hpv = L.at<PrfParams<NL>>(host, HB_MXP_PV);
            T.hrecs = L.at<void>(host, HB_MXP_PROOFS);
            T.hmx = L.at<MxRec<NL>>(host, HB_MXP_RECS);
            jobs_sec = HB_MXP_JOBS;
            T.data_off = L.off[HB_MXP_DATA];
            CHECK(hb_mixed_sum_wgs(Sv.data(), np, L.at<HbMxWg>(host, HB_MXP_SUMWG)) == cols);
            CHECK(hb_mixed_mont_wgs(nv.data(), np, L.at<HbMxWg>(host, HB_MXP_MONTWG)) == nmwg);
        } else {
            T.hpidx = L.at<PrfParams<2>>(host, HB_CMP_PIDX);
            T.hpv = L.at<PrfParams<NL>>(host, HB_CMP_PV);
            T.hitems = L.at<CpvItem>(host, HB_CMP_ITEMS);
            T.hrecs = L.at<void>(host, HB_CMP_PROOFS);
            T.hmx = L.at<MxRec<NL>>(host, HB_CMP_RECS);
            jobs_sec = HB_CMP_JOBS;
            T.data_off = L.off[HB_CMP_DATA];
            CHECK(hb_mixed_sum_wgs(Sv.data(), np, L.at<HbMxWg>(host, HB_CMP_SUMWG)) == cols);
            CHECK(hb_mixed_mont_wgs(nv.data(), np, L.at<HbMxWg>(host, HB_CMP_MONTWG)) == nmwg);
        }
        T.hjobs = L.at<PbWaveJob>(host, jobs_sec);
        if (cxx && nj) memcpy(host + L.off[jobs_sec], plan.jobs.data(), (size_t)(nj * sizeof(HbCbJob)));
        if (side == 0) {
            if (mixed)
                ref_prove_mixed<NL>(T, cxx, descs.data(), MC, nr, data_dev, tags_dev, ubase.data(), col0, np, O[0]);
            else
                ref_prove_one<NL>(T, cxx, items[0].P->pi, items[0].S, key_len, data_dev, tags_dev, plain.data(), ubase.data(), np,
                                  O[0]);
        } else if (mixed) {
            const ProveMixed V = {descs.data(), &cls, &MC};
            new_prove<NL>(T, cxx, true, V, nr, flags, ubase.data(), np, O[1]);
            new_prove_recs<NL>(T, V, col0, np);
        } else {
            const ProveOne V = {plain.data(), np, items[0].P->be.data(), items[0].P->be.size(), items[0].P->pi, items[0].S,
                                key_len,      key_len};
            new_prove<NL>(T, cxx, false, V, nr, flags, ubase.data(), np, O[1]);
        }
    }
    CHECK(O[0].status == 0 && O[1].status == 0);
    CHECK(memcmp(buf[0], buf[1], (size_t)L.up_bytes) == 0);
    CHECK(O[0].ddata == O[1].ddata && O[0].dtags == O[1].dtags && O[0].load16 == O[1].load16);
    CHECK(O[0].cursor == L.up_bytes && O[1].cursor == L.up_bytes);
    if (!cxx) CHECK(O[0].njobs == nj && O[1].njobs == nj);
    for (int v : O[1].load16) ++(v ? g_seen.load16_set : g_seen.load16_clear);
    free(buf[0]);
    free(buf[1]);
}

// ------------------------------------------------------------------ verify
template <int NL>
struct VerifyTables {
    PrfParams<2> *hpidx;
    PrfParams<NL> *hprf;
    CpvItem *hitems;      // cxx
    VbProof *hproofs;
    MxRec<NL> *hmx;       // many owners
    VbWaveJob *hjobs;     // PySwizzle
    u32 *hmu;
};

// verify_many_impl / cxx_verify_many_impl
template <int NL>
static void ref_verify_one(const VerifyTables<NL> &T, bool cxx, const PrfParams<NL> &P0, const PrimeInfo &pi, u32 S,
                           size_t key_len, size_t chal_key_len, const hb_verify_desc *proofs, const u64 *ubase, u64 np, Out &O) {
    const int nr = aes_rounds(key_len);
    const uint8_t one1 = 1;
    const uint8_t one16[16] = {1};
    RangeCache<2> PI0;
    RangeCache<NL> PV0;
    for (u64 f = 0; f < np; ++f) {
        const hb_verify_desc &D = proofs[f];
        const u64 n = cxx ? (D.chunks >= D.state_chunks ? D.state_chunks : D.chunks) : D.chunks;
        const u64 nstate = D.state_chunks ? D.state_chunks : 1;
        const uint8_t *vm = n ? D.vmax_be : cxx ? one16 : &one1;
        const size_t vl = n ? (size_t)D.vmax_len : cxx ? sizeof one16 : 1;
        if (!cxx) {
            if (!PI0.get(D.chal_key, chal_key_len, nstate) || !PV0.get(D.chal_key, chal_key_len, vm, vl)) {
                O.status = 1;
                return;
            }
            AesKey kf, ka, kc;
            if (!aes_expand(D.f_key, key_len, kf) || !aes_expand(D.alpha_key, key_len, ka) ||
                !aes_expand(D.chal_key, chal_key_len, kc)) {
                O.status = 1;
                return;
            }
            if (kf.nr != nr || ka.nr != nr || kc.nr != nr) {
                O.status = 2;
                return;
            }
            schedule<2>(PI0.tmpl, kc, T.hpidx[f]);
            schedule<NL>(P0, kf, T.hprf[3 * f + HB_VB_IDXF]);
            schedule<NL>(PV0.tmpl, kc, T.hprf[3 * f + HB_VB_V]);
            schedule<NL>(P0, ka, T.hprf[3 * f + HB_VB_ALPHA]);
            T.hproofs[f] = VbProof{ubase[f], (u32)D.chunks, 0u};
        } else {
            if (!PI0.get(D.chal_key, chal_key_len, nstate) || !PV0.get(D.chal_key, chal_key_len, vm, vl) ||
                !schedule<2>(PI0.tmpl, D.chal_key, chal_key_len, nr, T.hpidx[f]) ||
                !schedule<NL>(PV0.tmpl, D.chal_key, chal_key_len, nr, T.hprf[3 * f + HB_CPV_PV]) ||
                !schedule<NL>(P0, D.f_key, key_len, nr, T.hprf[3 * f + HB_CPV_PF]) ||
                !schedule<NL>(P0, D.alpha_key, key_len, nr, T.hprf[3 * f + HB_CPV_PA])) {
                O.status = 1;
                return;
            }
            T.hitems[f] = CpvItem{ubase[f], D.state_chunks, (u32)n, D.chunks >= D.state_chunks ? HB_CPV_ALL : 0u};
            T.hproofs[f] = VbProof{ubase[f], (u32)n, 0u};
        }
        for (u32 j = 0; j < S; ++j) be_to_limbs(D.mu + (size_t)j * pi.tw, pi.tw, T.hmu + ((size_t)f * S + j) * NL, NL);
    }
    if (!cxx) {
        u64 j = 0;
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_IDXF, T.hproofs[f].chunks);
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_ALPHA, S);
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_V, T.hproofs[f].chunks);
        O.njobs = j;
    }
}

// verify_mixed_impl / cxx_verify_mixed_impl
template <int NL>
static void ref_verify_mixed(const VerifyTables<NL> &T, bool cxx, const hb_verify_mixed_desc *descs, const MixedCall &MC, int nr,
                             const u64 *ubase, const std::vector<u64> &slot0, u64 np, Out &O) {
    const size_t key_len = nr == 10 ? 16 : nr == 12 ? 24 : 32;
    const uint8_t one1 = 1;
    const uint8_t one16[16] = {1};
    RangeCache<2> PI0;
    RangeCache<NL> PV0, PP0;
    for (u64 f = 0; f < np; ++f) {
        const u64 i = f;
        const hb_verify_mixed_desc &X = descs[i];
        const hb_verify_desc &D = X.d;
        const PrimeInfo &pi = MC.pi[(size_t)i];
        const u32 S = (u32)X.sectors;
        const u64 n = cxx ? (D.chunks >= D.state_chunks ? D.state_chunks : D.chunks) : D.chunks;
        const u64 nstate = D.state_chunks ? D.state_chunks : 1;
        const uint8_t *vm = n ? D.vmax_be : cxx ? one16 : &one1;
        const size_t vl = n ? (size_t)D.vmax_len : cxx ? sizeof one16 : 1;
        if (!cxx) {
            if (!PI0.get(D.chal_key, key_len, nstate) || !PV0.get(D.chal_key, key_len, vm, vl) ||
                !PP0.get(D.f_key, key_len, X.p_be, (size_t)X.p_len)) {
                O.status = 1;
                return;
            }
            AesKey kf, ka, kc;
            if (!aes_expand(D.f_key, key_len, kf) || !aes_expand(D.alpha_key, key_len, ka) ||
                !aes_expand(D.chal_key, (size_t)X.chal_key_len, kc)) {
                O.status = 1;
                return;
            }
            if (kf.nr != nr || ka.nr != nr || kc.nr != nr) {
                O.status = 2;
                return;
            }
            schedule<2>(PI0.tmpl, kc, T.hpidx[f]);
            schedule<NL>(PP0.tmpl, kf, T.hprf[3 * f + HB_VB_IDXF]);
            schedule<NL>(PV0.tmpl, kc, T.hprf[3 * f + HB_VB_V]);
            schedule<NL>(PP0.tmpl, ka, T.hprf[3 * f + HB_VB_ALPHA]);
            T.hproofs[f] = VbProof{ubase[f], (u32)D.chunks, 0u};
        } else {
            if (!PI0.get(D.chal_key, key_len, nstate) || !PV0.get(D.chal_key, key_len, vm, vl) ||
                !PP0.get(D.f_key, key_len, X.p_be, (size_t)X.p_len) ||
                !schedule<2>(PI0.tmpl, D.chal_key, key_len, nr, T.hpidx[f]) ||
                !schedule<NL>(PV0.tmpl, D.chal_key, key_len, nr, T.hprf[3 * f + HB_CPV_PV]) ||
                !schedule<NL>(PP0.tmpl, D.f_key, key_len, nr, T.hprf[3 * f + HB_CPV_PF]) ||
                !schedule<NL>(PP0.tmpl, D.alpha_key, key_len, nr, T.hprf[3 * f + HB_CPV_PA])) {
                O.status = 1;
                return;
            }
            T.hitems[f] = CpvItem{ubase[f], D.state_chunks, (u32)n,
                                  (D.chunks >= D.state_chunks ? HB_CPV_ALL : 0u) | (u32)slot0[(size_t)f] << HB_CMX_SLOT_SHIFT};
            T.hproofs[f] = VbProof{ubase[f], (u32)n, 0u};
        }
        fill_rec<NL>(MC.primes.primes[MC.prime_of[(size_t)i]], pi, S, 0, slot0[(size_t)f], T.hmx[f]);
        for (u32 j = 0; j < S; ++j) be_to_limbs(D.mu + (size_t)j * pi.tw, pi.tw, T.hmu + ((size_t)slot0[(size_t)f] + j) * NL, NL);
    }
    if (!cxx) {
        u64 j = 0;
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_IDXF, T.hproofs[f].chunks);
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_ALPHA, (u64)descs[f].sectors);
        for (u64 f = 0; f < np; ++f) push_jobs16(T.hjobs, j, f, HB_VB_V, T.hproofs[f].chunks);
        O.njobs = j;
    }
}

template <int NL, class View>
static void new_verify(const VerifyTables<NL> &T, bool cxx, bool mixed, const View &V, int nr, const PrfParams<NL> *P0,
                       const u64 *ubase, const std::vector<u64> &slot0, u64 np, Out &O) {
    uint8_t *host = (uint8_t *)T.hpidx;   // offsets from the first table
    VerifyFill<NL> F(host, 0, (u64)((uint8_t *)T.hprf - host), (u64)((uint8_t *)T.hmu - host), nr, cxx, P0);
    for (u64 f = 0; f < np; ++f) {
        const hb_verify_desc &D = V.d(f);
        const u64 n = cxx ? cxx_verify_chunks(D) : D.chunks;
        if (HbPvStatus st = F.entry(V, f, f, n, mixed ? slot0[(size_t)f] : f * V.S(f))) {
            O.status = st == HB_PV_ROUNDS ? 2 : 1;
            return;
        }
        if (cxx)
            T.hitems[f] = CpvItem{ubase[f], D.state_chunks, (u32)n,
                                  (cxx_all(D) ? HB_CPV_ALL : 0u) | (mixed ? (u32)slot0[(size_t)f] << HB_CMX_SLOT_SHIFT : 0u)};
        T.hproofs[f] = VbProof{ubase[f], (u32)n, 0u};
    }
    if (!cxx) O.njobs = verify_queue(T.hjobs, T.hproofs, np, [&](u64 f) { return (u64)V.S(f); });
}

template <int NL>
static void verify_case(std::vector<Item> &items, bool cxx, bool mixed, size_t key_len) {
    const u64 np = items.size();
    const HbBatchSizes z = sizes<NL>();
    const u64 rec = sizeof(MxRec<NL>);
    const int nr = aes_rounds(key_len);
    std::vector<hb_verify_mixed_desc> descs((size_t)np);
    std::vector<hb_verify_desc> plain((size_t)np);
    std::vector<u64> cls((size_t)np), ubase((size_t)np), slot0;
    std::vector<u32> Sv((size_t)np);
    std::vector<HbCbItemReq> req((size_t)np);
    MixedCall MC;
    u64 terms = 0, nj = 0;
    for (u64 f = 0; f < np; ++f) {
        Item &I = items[(size_t)f];
        hb_verify_mixed_desc &X = descs[(size_t)f];
        X.p_be = I.P->be.data();
        X.p_len = I.P->be.size();
        X.sectors = I.S;
        X.key_len = X.chal_key_len = key_len;
        X.d = hb_verify_desc{I.fkey.data(), I.akey.data(), I.key.data(), I.state_chunks, I.chunks,
                             I.chunks ? I.vmax.data() : nullptr, I.chunks ? I.vmax.size() : 0, I.mu.data(), I.out.data()};
        plain[(size_t)f] = X.d;
        cls[(size_t)f] = f;
        MC.prime_of.push_back(MC.primes.get(X.p_be, (size_t)X.p_len, NL));
        MC.pi.push_back(I.P->pi);
        const u64 eff = cxx ? cxx_verify_chunks(X.d) : X.d.chunks;
        ubase[(size_t)f] = terms;
        terms += eff;
        Sv[(size_t)f] = I.S;
        if (!cxx) nj += ((u64)I.S + 15) / 16 + 2 * ((eff + 15) / 16);
        req[(size_t)f].n[HB_CB_V] = req[(size_t)f].n[HB_CB_IDXF] = eff;
        req[(size_t)f].n[HB_CB_ALPHA] = I.S;
        req[(size_t)f].aes[HB_CB_V] = eff ? (byte_count(X.d.vmax_be, (size_t)X.d.vmax_len) + 15) / 16 : 1;
        req[(size_t)f].aes[HB_CB_IDXF] = req[(size_t)f].aes[HB_CB_ALPHA] = (I.P->pi.tw + 15) / 16;
        req[(size_t)f].units = eff;
        if (!eff) ++g_seen.no_chunks;
        if (cxx && cxx_all(X.d)) ++g_seen.all_verify;
    }
    HbCbPlan plan;
    if (cxx) {
        plan = hb_cbatch_plan(req.data(), np, ~0ull, ~0ull, ~0ull);
        CHECK(plan.groups.size() == 1 && plan.groups[0].nitems == np);
        nj = plan.groups[0].njobs;
    }
    const u64 slots = hb_mixed_prefix(Sv.data(), np, 0, slot0);
    const HbArena L = !mixed ? hb_verify_arena(z, cxx, np, nj, terms, items[0].S)
                      : cxx  ? hb_cmverify_arena(z, rec, np, nj, terms, slots)
                             : hb_mverify_arena(z, rec, np, nj, terms, slots);
    const u32 down = !mixed ? (u32)HB_VER_RES : cxx ? (u32)HB_CMV_RES : (u32)HB_MXV_RES;
    const u64 dbytes = L.total - L.off[down];
    const size_t size = (size_t)(L.up_bytes > dbytes ? L.up_bytes : dbytes);
    // the one-prime calls' template under p (batch_begin)
    PrfParams<NL> P0;
    int n0 = 0;
    CHECK(make_prf<NL>(items[0].fkey.data(), key_len, items[0].P->be.data(), items[0].P->be.size(), P0, n0));
    strip(P0);
    Out O[2];
    uint8_t *buf[2];
    for (int side = 0; side < 2; ++side) {
        uint8_t *host = buf[side] = (uint8_t *)malloc(size ? size : 1);
        memset(host, 0xA5, size);
        VerifyTables<NL> T = {};
        u32 jobs_sec;
        if (!mixed) {
            T.hpidx = L.at<PrfParams<2>>(host, HB_VER_PIDX);
            T.hprf = L.at<PrfParams<NL>>(host, HB_VER_PRF);
            T.hitems = L.at<CpvItem>(host, HB_VER_ITEMS);
            T.hproofs = L.at<VbProof>(host, HB_VER_PROOFS);
            T.hmu = L.at<u32>(host, HB_VER_MU);
            jobs_sec = HB_VER_JOBS;
        } else if (!cxx) {
            T.hpidx = L.at<PrfParams<2>>(host, HB_MXV_PIDX);
            T.hprf = L.at<PrfParams<NL>>(host, HB_MXV_PRF);
            T.hproofs = L.at<VbProof>(host, HB_MXV_PROOFS);
            T.hmx = L.at<MxRec<NL>>(host, HB_MXV_RECS);
            T.hmu = L.at<u32>(host, HB_MXV_MU);
            jobs_sec = HB_MXV_JOBS;
        } else {
            T.hpidx = L.at<PrfParams<2>>(host, HB_CMV_PIDX);
            T.hprf = L.at<PrfParams<NL>>(host, HB_CMV_PRF);
            T.hitems = L.at<CpvItem>(host, HB_CMV_ITEMS);
            T.hproofs = L.at<VbProof>(host, HB_CMV_PROOFS);
            T.hmx = L.at<MxRec<NL>>(host, HB_CMV_RECS);
            T.hmu = L.at<u32>(host, HB_CMV_MU);
            jobs_sec = HB_CMV_JOBS;
        }
        T.hjobs = L.at<VbWaveJob>(host, jobs_sec);
        if (cxx && nj) memcpy(host + L.off[jobs_sec], plan.jobs.data(), (size_t)(nj * sizeof(HbCbJob)));
        if (side == 0) {
            if (mixed)
                ref_verify_mixed<NL>(T, cxx, descs.data(), MC, nr, ubase.data(), slot0, np, O[0]);
            else
                ref_verify_one<NL>(T, cxx, P0, items[0].P->pi, items[0].S, key_len, key_len, plain.data(), ubase.data(), np, O[0]);
        } else if (mixed) {
            const VerifyMixed V = {descs.data(), &cls, &MC};
            new_verify<NL>(T, cxx, true, V, nr, nullptr, ubase.data(), slot0, np, O[1]);
            for (u64 f = 0; f < np; ++f) fill_rec<NL>(V.prime(f), V.pi(f), V.S(f), 0, slot0[(size_t)f], T.hmx[f]);
        } else {
            const VerifyOne V = {plain.data(), np, items[0].P->be.data(), items[0].P->be.size(), items[0].P->pi, items[0].S,
                                 key_len,      key_len};
            new_verify<NL>(T, cxx, false, V, nr, &P0, ubase.data(), slot0, np, O[1]);
        }
    }
    CHECK(O[0].status == 0 && O[1].status == 0);
    CHECK(memcmp(buf[0], buf[1], (size_t)L.up_bytes) == 0);
    if (!cxx) CHECK(O[0].njobs == nj && O[1].njobs == nj);
    // the end cursor of a verify's upload: mu is its last section
    CHECK(L.off[!mixed ? (u32)HB_VER_MU : cxx ? (u32)HB_CMV_MU : (u32)HB_MXV_MU] + (mixed ? slots : np * items[0].S) * NL * 4 ==
          L.up_bytes);
    free(buf[0]);
    free(buf[1]);
}

// ------------------------------------------------------------------ the sweep
static const u64 kChunks[] = {1, 15, 16, 17, 33};
static const u32 kS[] = {1, 3, 16, 17};
static const u64 kLens[] = {0, 95, 200};
static const u64 kTags[] = {1, 7, 40};
static const u64 kState[] = {1, 7, 40, 0};

static Item make_item(const Prime *P, u32 S, size_t key_len, u64 chunks, u64 ntags, u64 state_chunks, u64 len, bool vmax_p,
                      bool dev_odd) {
    Item I;
    I.P = P;
    I.S = S;
    I.chunks = chunks;
    I.ntags = ntags;
    I.state_chunks = state_chunks;
    I.len = len;
    I.key = bytes(key_len);
    I.fkey = bytes(key_len);
    I.akey = bytes(key_len);
    I.vmax = vmax_p ? P->be : std::vector<uint8_t>(1, 1);
    I.data = bytes((size_t)len);
    I.tags = bytes((size_t)(ntags * P->pi.tw));
    I.mu = bytes((size_t)S * P->pi.tw);
    I.out.assign((size_t)(S + 1) * P->pi.tw, 0);
    I.dev_data = (const uint8_t *)(uintptr_t)(0x7e0000001000ull + (dev_odd ? 1 : 0));
    I.dev_tags = (const uint8_t *)(uintptr_t)0x7e0000100000ull;
    ++(vmax_p ? g_seen.vmax_p : g_seen.vmax_1);
    ++(dev_odd ? g_seen.dev_odd : g_seen.dev_even);
    return I;
}

template <int NL>
static void sweep(const std::vector<const Prime *> &primes) {
    u32 t = 0;
    for (int cxx = 0; cxx < 2; ++cxx)
        for (int mixed = 0; mixed < 2; ++mixed)
            for (size_t key_len = 16; key_len <= 32; key_len += 8)
                for (u64 np = 1; np <= 3; ++np)
                    for (u32 rep = 0; rep < 20; ++rep, ++t) {
                        // neighbours: every other repetition repeats proof 0's ranges
                        // (RangeCache hit), the others move on (miss); many owners:
                        // primes and S change from proof to proof (ragged col0 / slot0)
                        const bool same = rep % 2 == 0;
                        std::vector<Item> pv, vv;
                        for (u64 f = 0; f < np; ++f) {
                            const u32 s = same ? t : t + 7 * (u32)f;
                            const Prime *P = primes[(mixed ? t / 3 + f : t / 3) % primes.size()];
                            const u32 S = kS[(mixed ? t + 3 * f : t) % 4];
                            const u64 chunks = kChunks[(t + f) % 5];
                            pv.push_back(make_item(P, S, key_len, chunks, kTags[s % 3], 0, kLens[(t + f) % 3], (s / 2) % 2 == 0,
                                                   (t / 5) % 2 == 1));
                            vv.push_back(make_item(P, S, key_len, (t + f) % 6 == 5 ? 0 : chunks, 0, kState[s % 4], 0, (s / 2) % 2 == 0,
                                                   false));
                            if (f) {
                                ++(same ? g_seen.range_hit : g_seen.range_miss);
                                if (mixed && (pv[f].P != pv[f - 1].P || pv[f].S != pv[f - 1].S)) ++g_seen.ragged;
                            }
                        }
                        snprintf(g_case, sizeof g_case, "NL %d cxx %d mixed %d key_len %zu np %llu rep %u", NL, cxx, mixed, key_len,
                                 (unsigned long long)np, rep);
                        const int res = (int)(t % 4);   // residency: data, tags on the device
                        prove_case<NL>(pv, cxx != 0, mixed != 0, key_len, (res & 1) != 0, (res & 2) != 0);
                        verify_case<NL>(vv, cxx != 0, mixed != 0, key_len);
                    }
}

int main() {
    const Prime q255 = prime_of(255, 19), q256 = p256();            // ss 31, tw 32: never load16; ss = tw = 4 NL
    const Prime q1024 = prime_of(1024, 105), q607 = prime_of(607, 1);   // ss = tw = 4 NL; ss 75, tw 76
    CHECK(q255.pi.ss == 31 && q255.pi.tw == 32 && q256.pi.ss == 32 && q1024.pi.ss == 128 && q1024.pi.tw == 128 &&
          q607.pi.nl == 32 && q607.pi.ss == 75 && q607.pi.tw == 76);
    CHECK(aes_key_len(aes_rounds(16)) == 16 && aes_key_len(aes_rounds(24)) == 24 && aes_key_len(aes_rounds(32)) == 32);
    CHECK(pv_bound(~0ull, 1ull << 31) == 1ull << 31 && pv_bound(5, 1ull << 31) == 5 && pv_bound(~0ull, 0xffffffffull) == 0xffffffffull);
    sweep<8>({&q255, &q256});
    sweep<32>({&q1024, &q607});
    snprintf(g_case, sizeof g_case, "coverage");
    CHECK(g_seen.load16_set > 0 && g_seen.load16_clear > 0 && g_seen.range_hit > 0 && g_seen.range_miss > 0 && g_seen.ragged > 0 &&
          g_seen.all_prove > 0 && g_seen.all_verify > 0 && g_seen.no_chunks > 0 && g_seen.vmax_p > 0 && g_seen.vmax_1 > 0 &&
          g_seen.dev_odd > 0 && g_seen.dev_even > 0);
    printf("ok %ld\n", g_checks);
    return 0;
}
