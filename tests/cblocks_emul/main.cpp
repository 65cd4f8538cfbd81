// Walks the pure host header of the cxx listed-block encode
// (heartbeat_amd/csrc/hb_cblocks_host.hpp): the index-range check and its
// place after the descriptor checks, the split of the lists into segments and
// groups under forced block and byte caps, the MAC count of a segment whose
// last block is empty, each group's queue of wave-jobs, and the fill of a
// group's staging buffer -- key schedules, file records, wave-jobs, MAC
// workgroups, narrowed indices, host blocks -- over a heap block of exactly
// the uploaded size.  Built with -fsanitize=address,undefined and run by
// tests/test_cblocks_host.py.  Exit status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "hb_cblocks_host.hpp"

using namespace hbhost;

static int g_checks = 0, g_bad = 0;

static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    ++g_checks;
    if (!ok) {
        ++g_bad;
        if (g_bad < 50) printf("FAIL %s (%lld, %lld)\n", what, a, b);
    }
}

static uint64_t g_x = 0x13198a2e03707344ull;
static uint64_t rnd() {
    g_x = g_x * 6364136223846793005ull + 1442695040888963407ull;
    return g_x >> 17;
}

static void check_order() {
    const uint64_t C = 64;
    uint8_t k1[32] = {1}, k2[32] = {2}, data[256] = {0}, tags[256];
    uint64_t idx[4] = {7, 0xffffffffull, 7, 0};
    auto good = [&]() { return hb_blocks_desc{k1, k2, idx, 4, data, 4 * C - 5, tags}; };
    std::string msg;
    std::vector<hb_blocks_desc> d(5, good());
    expect(hb_cblocks_check(d.data(), d.size(), C, msg) == 0 && msg.empty(), "five good files: 0, 2^32 - 1 and a repeat pass");
    // the first index of 2^32 or above, by file and list position
    uint64_t wide[4] = {1, 1ull << 32, 3, ~0ull};
    d[3].indices = wide;
    msg.clear();
    expect(hb_cblocks_check(d.data(), d.size(), C, msg) == HB_EUNSUPPORTED, "2^32 is refused as unsupported");
    expect(msg == "file 3: index 4294967296 (listed block 1) does not fit the cxx prf's unsigned int", "the message names file, index and position");
    uint64_t wide2[4] = {1, 2, 3, ~0ull};
    d[1].indices = wide2;
    hb_cblocks_check(d.data(), d.size(), C, msg);
    expect(msg.find("file 1: index 18446744073709551615 (listed block 3)") == 0, "the first file with a wide index");
    // every descriptor check comes before any index check: a later file's bad descriptor wins
    d[4].tags = nullptr;
    expect(hb_cblocks_check(d.data(), d.size(), C, msg) == HB_EINVAL && msg == "file 4: tags buffer is NULL",
           "descriptors before indices");
    d[4] = good();
    d[4].len = 1;
    expect(hb_cblocks_check(d.data(), d.size(), C, msg) == HB_EINVAL && msg.find("file 4: len is outside") == 0, "len before indices");
    d[4] = good();
    // an empty list has no index to check, wide or not
    hb_blocks_desc e = {k1, k2, nullptr, 0, nullptr, 0, nullptr};
    d[1] = e;
    d[3] = e;
    expect(hb_cblocks_check(d.data(), d.size(), C, msg) == 0, "empty lists pass");
}

static void mac_counts() {
    const uint64_t C = 310;
    expect(hb_cblocks_mac(0, C, 1) == 0, "one empty block: no MAC block");
    expect(hb_cblocks_mac(1, C, 1) == 1 && hb_cblocks_mac(C, C, 1) == 1, "one block with bytes");
    expect(hb_cblocks_mac(4 * C, C, 5) == 4, "five blocks, the last empty: four");
    expect(hb_cblocks_mac(4 * C + 1, C, 5) == 5 && hb_cblocks_mac(5 * C, C, 5) == 5, "five blocks with bytes in the last");
    expect(hb_cblocks_mac(4 * C, C, 4) == 4, "four whole blocks");
}

template <int NL>
static HbBatchSizes sizes() {
    HbBatchSizes z;
    memset(&z, 0, sizeof z);
    z.prf2 = sizeof(PrfParams<2>);
    z.prf = sizeof(PrfParams<NL>);
    z.limbs = NL * 4;
    z.file = sizeof(BatchFile);
    z.wg = sizeof(BatchMacWg);
    return z;
}

struct Batch {
    std::vector<std::vector<uint8_t>> fk, ak, data, tags;
    std::vector<std::vector<uint64_t>> idx;
    std::vector<hb_blocks_desc> d;
    void set(size_t f) {
        d[f] = hb_blocks_desc{fk[f].data(), ak[f].data(), idx[f].empty() ? nullptr : idx[f].data(), idx[f].size(),
                              data[f].empty() ? nullptr : data[f].data(), data[f].size(), tags[f].empty() ? nullptr : tags[f].data()};
    }
};

// nf files with random lists; the last listed block of a file may be short or empty
static void make_batch(Batch &B, uint64_t nf, uint64_t C, uint32_t tw, uint64_t max_blocks, size_t key_len) {
    B.fk.resize(nf), B.ak.resize(nf), B.data.resize(nf), B.tags.resize(nf), B.idx.resize(nf), B.d.resize(nf);
    for (uint64_t f = 0; f < nf; ++f) {
        const uint64_t nb = rnd() % 4 == 0 ? 0 : rnd() % (max_blocks + 1);
        uint64_t len = 0;
        if (nb) {
            const uint64_t k = rnd() % 4;
            len = (nb - 1) * C + (k == 0 ? 0 : k == 1 ? C : rnd() % (C + 1));
        }
        B.fk[f].assign(key_len, 0), B.ak[f].assign(key_len, 0);
        for (size_t i = 0; i < key_len; ++i) B.fk[f][i] = (uint8_t)rnd(), B.ak[f][i] = (uint8_t)rnd();
        B.data[f].resize(len);
        for (auto &b : B.data[f]) b = (uint8_t)rnd();
        B.idx[f].resize(nb);
        for (auto &i : B.idx[f]) i = rnd() % 3 == 0 ? 0xffffffffull - rnd() % 5 : (rnd() & 0xffffffffull) >> (rnd() % 32);
        B.tags[f].assign(nb * tw, 0xee);
        B.set(f);
    }
}

static uint64_t seg_len_of(const Batch &B, const HbBlkSeg &X, uint64_t C) {
    return hb_blocks_seg_len(B.d[X.file].len, C, X.first, X.count);
}

static void check_plan(const Batch &B, const HbCblkPlan &P, const HbBatchSizes &z, const BlkShape &E, uint64_t cap_blocks,
                       uint64_t cap_bytes) {
    const HbBlkPlan &Q = P.blk;
    size_t s = 0;
    for (uint64_t f = 0; f < B.d.size(); ++f) {
        uint64_t at = 0;
        while (at < B.d[f].nblocks) {
            expect(s < Q.segs.size() && Q.segs[s].file == f && Q.segs[s].first == at && Q.segs[s].count >= 1,
                   "segments cover the lists in order", (long long)f, (long long)at);
            if (s >= Q.segs.size()) return;
            // the empty last block belongs to the list's last segment only
            const uint64_t slen = seg_len_of(B, Q.segs[s], E.C), mac = hb_cblocks_mac(slen, E.C, Q.segs[s].count);
            const bool last_seg = at + Q.segs[s].count == B.d[f].nblocks;
            const bool empty_last = B.d[f].len == (B.d[f].nblocks - 1) * E.C;
            expect(mac == Q.segs[s].count - (last_seg && empty_last ? 1 : 0), "a segment's MAC count", (long long)f, (long long)at);
            at += Q.segs[s++].count;
        }
        expect(at == B.d[f].nblocks, "a list is covered exactly");
    }
    expect(s == Q.segs.size(), "no segment beyond the lists");
    expect(P.cb.groups.size() == Q.groups.size() && P.cb.order.size() == Q.segs.size(), "one queue per group");
    uint64_t seg = 0, job = 0;
    for (size_t g = 0; g < Q.groups.size(); ++g) {
        const HbBlkGroup &G = Q.groups[g];
        expect(G.seg0 == seg && G.nsegs >= 1, "groups partition the segments");
        uint64_t blocks = 0, bytes = 0, nj = 0;
        for (uint64_t k = 0; k < G.nsegs; ++k) {
            const HbBlkSeg &X = Q.segs[(size_t)(G.seg0 + k)];
            blocks += X.count;
            bytes += hb_cblocks_cost(z, E, seg_len_of(B, X, E.C), X.count);
            nj += hb_cblocks_jobs(E, X.count);
        }
        expect(blocks == G.blocks && bytes == G.bytes, "a group's totals");
        expect(G.blocks <= cap_blocks, "the block cap holds", (long long)G.blocks, (long long)cap_blocks);
        expect(G.bytes <= cap_bytes || G.blocks == 1, "the byte cap holds unless one block is alone");
        // the queue: every evaluation of every segment once, under its kind, fuller wave-jobs first
        const HbCbGroup &J = P.cb.groups[g];
        expect(J.job0 == job && J.njobs == nj && J.item0 == G.seg0 && J.nitems == G.nsegs, "a group's queue", (long long)J.njobs,
               (long long)nj);
        std::vector<std::vector<int>> seenF(G.nsegs), seenA(G.nsegs);
        for (uint64_t k = 0; k < G.nsegs; ++k) seenF[k].assign(Q.segs[(size_t)(G.seg0 + k)].count, 0), seenA[k].assign(E.S, 0);
        for (uint64_t j = 0; j < J.njobs; ++j) {
            const HbCbJob &W = P.cb.jobs[(size_t)(J.job0 + j)];
            expect(W.item < G.nsegs && (W.kind == HB_CB_F || W.kind == HB_CB_ALPHA) && W.count >= 1 && W.count <= HB_CB_JOB,
                   "a wave-job names a segment of its group and a kind");
            if (W.item >= G.nsegs) continue;
            std::vector<int> &seen = W.kind == HB_CB_F ? seenF[W.item] : seenA[W.item];
            expect((uint64_t)W.first + W.count <= seen.size(), "a wave-job stays inside its segment");
            for (uint64_t e = W.first; e < (uint64_t)W.first + W.count && e < seen.size(); ++e) ++seen[e];
            if (j) expect(P.cb.jobs[(size_t)(J.job0 + j - 1)].count >= W.count, "fuller wave-jobs first");
        }
        for (uint64_t k = 0; k < G.nsegs; ++k) {
            for (int v : seenF[k]) expect(v == 1, "every F evaluation once");
            for (int v : seenA[k]) expect(v == 1, "every alpha evaluation once");
        }
        seg += G.nsegs;
        job += J.njobs;
    }
    expect(seg == Q.segs.size() && job == P.cb.jobs.size(), "every segment and wave-job has a group");
}

static void forced_split() {
    const HbBatchSizes z = sizes<32>();
    const BlkShape E = {1280, 10, 128, 4, false, false, true};
    Batch B;
    make_batch(B, 1, E.C, E.tw, 0, 32);
    // 50 blocks whose last is empty, under a cap of 20: 20 + 20 + 10, the MAC counts 20, 20, 9
    B.idx[0].assign(50, 5);
    B.data[0].assign(49 * E.C, 1);
    B.tags[0].assign(50 * E.tw, 0);
    B.set(0);
    const HbCblkPlan P = hb_cblocks_plan(B.d.data(), 1, z, E, 20, HB_BATCH_BYTES);
    expect(P.blk.groups.size() == 3 && P.blk.segs.size() == 3, "50 blocks under a cap of 20: three groups", (long long)P.blk.groups.size());
    if (P.blk.segs.size() == 3) {
        expect(P.blk.segs[0].count == 20 && P.blk.segs[1].count == 20 && P.blk.segs[2].count == 10 && P.blk.segs[2].first == 40, "20 + 20 + 10");
        expect(hb_cblocks_mac(seg_len_of(B, P.blk.segs[0], E.C), E.C, 20) == 20 && hb_cblocks_mac(seg_len_of(B, P.blk.segs[1], E.C), E.C, 20) == 20 &&
                   hb_cblocks_mac(seg_len_of(B, P.blk.segs[2], E.C), E.C, 10) == 9,
               "MAC counts 20, 20, 9");
        const HbBlkTotals T = hb_cblocks_totals(B.d.data(), P.blk, P.blk.groups[2], E, P.cb.groups[2].njobs);
        expect(T.nwg == 3 && T.nj == 2, "the last group: 9 MAC blocks in workgroups of 4, one alpha and one F wave-job", (long long)T.nwg,
               (long long)T.nj);
    }
    check_plan(B, P, z, E, 20, HB_BATCH_BYTES);
    // a list that is only one empty block: a group without any MAC workgroup
    Batch B1;
    make_batch(B1, 1, E.C, E.tw, 0, 32);
    B1.idx[0].assign(1, 77);
    B1.tags[0].assign(E.tw, 0);
    B1.set(0);
    const HbCblkPlan P1 = hb_cblocks_plan(B1.d.data(), 1, z, E, ~0ull, HB_BATCH_BYTES);
    expect(P1.blk.groups.size() == 1, "one empty block: one group");
    if (P1.blk.groups.size() == 1) {
        const HbBlkTotals T = hb_cblocks_totals(B1.d.data(), P1.blk, P1.blk.groups[0], E, P1.cb.groups[0].njobs);
        expect(T.nwg == 0 && T.nj == 2 && T.dbytes == 0, "no MAC workgroup, two wave-jobs, no data");
    }
    // 129 blocks: three F wave-jobs of 64, 64 and 1
    Batch B2;
    make_batch(B2, 1, E.C, E.tw, 0, 32);
    B2.idx[0].assign(129, 3);
    B2.data[0].assign(129 * E.C, 2);
    B2.tags[0].assign(129 * E.tw, 0);
    B2.set(0);
    const HbCblkPlan P2 = hb_cblocks_plan(B2.d.data(), 1, z, E, ~0ull, HB_BATCH_BYTES);
    expect(P2.cb.jobs.size() == 4 && P2.cb.jobs[0].count == 64 && P2.cb.jobs[1].count == 64 && P2.cb.jobs[3].count == 1, "129 blocks: 64, 64, (alpha 10), 1");
    check_plan(B2, P2, z, E, ~0ull, HB_BATCH_BYTES);
    // a byte cap below one block's cost: every block alone
    const HbCblkPlan R = hb_cblocks_plan(B.d.data(), 1, z, E, ~0ull, 1);
    expect(R.blk.groups.size() == 50 && R.blk.segs.size() == 50, "a byte cap of 1: fifty groups of one block");
    check_plan(B, R, z, E, ~0ull, 1);
}

template <int NL>
static void fills(size_t key_len) {
    const HbBatchSizes z = sizes<NL>();
    const int nr = aes_rounds(key_len);
    uint8_t p_be[NL * 4];
    for (auto &b : p_be) b = (uint8_t)(rnd() | 1);
    p_be[0] |= 0x80;
    for (int round = 0; round < 40; ++round) {
        const uint32_t S = 1 + (uint32_t)(rnd() % (round % 7 == 0 ? 150 : 40)), ss = NL * 4 - 1, tw = NL * 4;
        BlkShape E = {(uint64_t)ss * S, S, tw, 1 + (uint32_t)(rnd() % 9), (round & 1) != 0, (round & 2) != 0, false};
        Batch B;
        make_batch(B, 1 + rnd() % 7, E.C, tw, round % 8 == 0 ? 200 : 45, key_len);
        const uint64_t cap_blocks = round % 4 == 0 ? 1 + rnd() % 20 : ~0ull;
        const uint64_t cap_bytes = round % 5 == 0 ? 4000 + rnd() % 60000 : HB_BATCH_BYTES;
        const HbCblkPlan P = hb_cblocks_plan(B.d.data(), B.d.size(), z, E, cap_blocks, cap_bytes);
        check_plan(B, P, z, E, cap_blocks, cap_bytes);
        PrfParams<NL> P0;
        int n0 = 0;
        expect(make_prf<NL>(B.fk[0].data(), key_len, p_be, sizeof p_be, P0, n0) && n0 == nr, "range template");
        strip(P0);
        uint8_t *const dev = (uint8_t *)(uintptr_t)0x7f0000000000ull + 16 * (rnd() % 8);
        for (size_t g = 0; g < P.blk.groups.size(); ++g) {
            const HbBlkGroup &G = P.blk.groups[g];
            const HbBlkTotals T = hb_cblocks_totals(B.d.data(), P.blk, G, E, P.cb.groups[g].njobs);
            const HbArena L = hb_cblocks_arena(z, E, G, T);
            expect(L.n == 9 && L.total <= G.bytes + 16 * 9, "the arena is inside the group's cost", (long long)L.total, (long long)G.bytes);
            // exactly the uploaded bytes: a write past them is a sanitizer report
            std::vector<uint8_t> host((size_t)L.up_bytes, 0xa5);
            uint64_t bad = ~0ull;
            expect(hb_cblocks_fill<NL>(B.d.data(), P, g, E, L, P0, key_len, nr, host.data(), dev, bad), "fill");
            const PrfParams<NL> *hprf = L.at<PrfParams<NL>>(host.data(), HB_CBK_PRF);
            const BatchFile *hf = L.at<BatchFile>(host.data(), HB_CBK_FILES);
            const HbCbJob *hj = L.at<HbCbJob>(host.data(), HB_CBK_JOBS);
            const BatchMacWg *hw = L.at<BatchMacWg>(host.data(), HB_CBK_WGS);
            const uint32_t *hi = L.at<uint32_t>(host.data(), HB_CBK_IDX);
            uint64_t w = 0, fbase = 0, doff = L.off[HB_CBK_DATA], toff = L.off[HB_CBK_TAGS];
            for (uint64_t s = 0; s < G.nsegs; ++s) {
                const HbBlkSeg &X = P.blk.segs[(size_t)(G.seg0 + s)];
                const hb_blocks_desc &D = B.d[X.file];
                AesKey kf, ka;
                aes_expand(D.f_key, key_len, kf);
                aes_expand(D.alpha_key, key_len, ka);
                expect(memcmp(hprf[2 * s + HB_CB_F].rk, kf.rk, 16 * (size_t)(nr + 1)) == 0 &&
                           memcmp(hprf[2 * s + HB_CB_ALPHA].rk, ka.rk, 16 * (size_t)(nr + 1)) == 0,
                       "key schedules: f_key at kind F, alpha_key at kind alpha");
                expect(memcmp(hprf[2 * s].R, P0.R, sizeof P0.R) == 0 && hprf[2 * s + 1].nb == P0.nb && hprf[2 * s].topmask == P0.topmask,
                       "the schedules keep the template's range");
                const uint64_t slen = hb_blocks_seg_len(D.len, E.C, X.first, X.count), mac = hb_cblocks_mac(slen, E.C, X.count);
                const BatchFile &F = hf[s];
                expect(F.len == slen && F.nblocks == mac && F.fbase == fbase, "record: len, the MAC's nblocks, fbase");
                // the kernel's keep-tag rule picks exactly the blocks the MAC does not see
                for (uint64_t k = 0; k < X.count; ++k) expect((k * E.C >= F.len) == (k >= mac), "position k keeps F iff the MAC skips it");
                if (E.data_dev) {
                    expect(F.data == (D.data ? D.data + X.first * E.C : nullptr), "device data: the caller's pointer at the segment");
                } else {
                    expect(F.data == dev + doff, "host data: its place in the arena");
                    expect(slen == 0 || memcmp(host.data() + doff, D.data + X.first * E.C, (size_t)slen) == 0, "host data: the bytes");
                    doff += hb_up16(slen);
                }
                if (E.tags_dev) {
                    expect(F.tags == D.tags + X.first * tw, "device tags: the caller's pointer at the segment");
                } else {
                    expect(F.tags == dev + toff, "host-bound tags: their place in the arena");
                    toff += hb_up16(X.count * tw);
                }
                expect(!(F.flags & HB_BF_LOAD16), "load16 off for a shape that does not allow it");
                expect(((F.flags & HB_BF_TAGS4) != 0) == ((uintptr_t)F.tags % 4 == 0), "tags4");
                for (uint64_t k = 0; k < X.count; ++k) expect(hi[fbase + k] == (uint32_t)D.indices[X.first + k] && D.indices[X.first + k] >> 32 == 0, "indices: the segment's slice, narrowed");
                for (uint64_t b = 0; b < mac; b += E.bpw, ++w) expect(hw[w].file == s && hw[w].first == b, "MAC workgroups over the MAC's blocks");
                fbase += X.count;
            }
            expect(w == T.nwg && fbase == G.blocks, "the tables add up");
            expect(T.nj == P.cb.groups[g].njobs && (T.nj == 0 || memcmp(hj, P.cb.jobs.data() + P.cb.groups[g].job0, (size_t)T.nj * sizeof(HbCbJob)) == 0),
                   "the group's queue, as planned");
            expect(E.data_dev || doff == L.off[HB_CBK_DATA] + T.dbytes, "the data cursor ends at the section's end");
            expect(doff <= L.up_bytes, "the data ends inside the upload");
            if (!E.tags_dev) {
                std::vector<uint8_t> down((size_t)T.tbytes);
                for (size_t k = 0; k < down.size(); ++k) down[k] = (uint8_t)(k * 7 + 1);
                hb_blocks_tags_out(B.d.data(), P.blk, G, E, down.data());
                uint64_t off = 0;
                for (uint64_t s = 0; s < G.nsegs; ++s) {
                    const HbBlkSeg &X = P.blk.segs[(size_t)(G.seg0 + s)];
                    expect(memcmp(B.tags[X.file].data() + X.first * tw, down.data() + off, (size_t)(X.count * tw)) == 0,
                           "tags back at the segment's place");
                    off += hb_up16(X.count * tw);
                }
            }
        }
        if (!P.blk.groups.empty() && round == 0) {
            const HbBlkGroup &G = P.blk.groups[0];
            const HbBlkTotals T = hb_cblocks_totals(B.d.data(), P.blk, G, E, P.cb.groups[0].njobs);
            const HbArena L = hb_cblocks_arena(z, E, G, T);
            std::vector<uint8_t> host((size_t)L.up_bytes);
            uint64_t bad = ~0ull;
            expect(!hb_cblocks_fill<NL>(B.d.data(), P, 0, E, L, P0, key_len, nr == 10 ? 12 : 10, host.data(), dev, bad) &&
                       bad == P.blk.segs[(size_t)G.seg0].file,
                   "a key of another round count");
        }
    }
}

int main() {
    check_order();
    mac_counts();
    forced_split();
    fills<8>(32);
    fills<8>(16);
    fills<32>(24);
    fills<32>(32);
    fills<64>(32);
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
