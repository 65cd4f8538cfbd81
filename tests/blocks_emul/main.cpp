// Walks the pure host header of the listed-block encode
// (heartbeat_amd/csrc/hb_blocks_host.hpp): the len bounds, the order of the
// descriptor checks and the file index in the message, the split of the lists
// into segments and groups (forced caps included), and the fill of a group's
// staging buffer -- key schedules, file records, wave-jobs, MAC workgroups,
// indices, host blocks -- over a heap block of exactly the uploaded size, and
// the tags' way back.  Built with -fsanitize=address,undefined and run by
// tests/test_blocks_host.py.  Exit status 0 and "ok <n>" on success.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "hb_blocks_host.hpp"

using namespace hbhost;

static int g_checks = 0, g_bad = 0;

static void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    ++g_checks;
    if (!ok) {
        ++g_bad;
        if (g_bad < 50) printf("FAIL %s (%lld, %lld)\n", what, a, b);
    }
}

static uint64_t g_x = 0x243f6a8885a308d3ull;
static uint64_t rnd() {
    g_x = g_x * 6364136223846793005ull + 1442695040888963407ull;
    return g_x >> 17;
}

static void len_bounds() {
    const uint64_t C = 310, M = ~0ull;
    expect(hb_blocks_len_ok(0, 0, C), "no blocks, no bytes");
    expect(!hb_blocks_len_ok(0, 1, C), "no blocks but bytes");
    expect(hb_blocks_len_ok(1, 0, C), "one empty block");
    expect(hb_blocks_len_ok(1, 1, C) && hb_blocks_len_ok(1, C - 1, C) && hb_blocks_len_ok(1, C, C), "one block up to C");
    expect(!hb_blocks_len_ok(1, C + 1, C), "one block above C");
    expect(!hb_blocks_len_ok(3, 2 * C - 1, C), "a short block before the last");
    expect(hb_blocks_len_ok(3, 2 * C, C) && hb_blocks_len_ok(3, 2 * C + 7, C) && hb_blocks_len_ok(3, 3 * C, C), "three blocks");
    expect(!hb_blocks_len_ok(3, 3 * C + 1, C), "three blocks above 3 C");
    // products past 2^64 must not wrap into acceptance
    expect(!hb_blocks_len_ok(M, 5, C), "2^64 - 1 blocks of 310 bytes");
    expect(!hb_blocks_len_ok(M / C + 2, M, C), "(nblocks - 1) C past 2^64");
    expect(hb_blocks_len_ok(M / C + 1, M, C), "nblocks C past 2^64, (nblocks - 1) C below len");
    expect(hb_blocks_len_ok(2, M, M - 1) && !hb_blocks_len_ok(2, M - 2, M - 1), "C near 2^64");
    for (int r = 0; r < 2000; ++r) {
        const uint64_t c = 1 + rnd() % 600, nb = rnd() % 9, len = rnd() % (10 * c);
        const bool want = nb == 0 ? len == 0 : (len >= (nb - 1) * c && len <= nb * c);
        expect(hb_blocks_len_ok(nb, len, c) == want, "len bounds against the plain formula", (long long)nb, (long long)len);
    }
}

static void check_order() {
    const uint64_t C = 64;
    uint8_t k1[32] = {1}, k2[32] = {2}, data[256] = {0}, tags[256];
    uint64_t idx[4] = {7, 3, 3, ~0ull};
    auto good = [&]() { return hb_blocks_desc{k1, k2, idx, 4, data, 4 * C - 5, tags}; };
    std::string msg;
    std::vector<hb_blocks_desc> d(5, good());
    expect(hb_blocks_check(d.data(), d.size(), C, msg) && msg.empty(), "five good files");
    hb_blocks_desc e = {k1, k2, nullptr, 0, nullptr, 0, nullptr};
    d[2] = e;
    expect(hb_blocks_check(d.data(), d.size(), C, msg), "an empty list needs no indices, data or tags");
    // one fault each, in file 3: the message names the file and the fault
    struct Case {
        const char *what;
        void (*spoil)(hb_blocks_desc &);
    };
    const Case cases[] = {
        {"file 3: a key is NULL", [](hb_blocks_desc &x) { x.f_key = nullptr; }},
        {"file 3: a key is NULL", [](hb_blocks_desc &x) { x.alpha_key = nullptr; }},
        {"file 3: indices is NULL", [](hb_blocks_desc &x) { x.indices = nullptr; }},
        {"file 3: len is outside [(nblocks - 1) * C, nblocks * C]", [](hb_blocks_desc &x) { x.len = 4 * 64 + 1; }},
        {"file 3: len is outside [(nblocks - 1) * C, nblocks * C]", [](hb_blocks_desc &x) { x.len = 3 * 64 - 1; }},
        {"file 3: len is outside [(nblocks - 1) * C, nblocks * C]", [](hb_blocks_desc &x) { x.nblocks = 0; }},
        {"file 3: tags buffer is NULL", [](hb_blocks_desc &x) { x.tags = nullptr; }},
        {"file 3: data buffer is NULL", [](hb_blocks_desc &x) { x.data = nullptr; }},
    };
    for (const Case &c : cases) {
        d[3] = good();
        c.spoil(d[3]);
        msg.clear();
        expect(!hb_blocks_check(d.data(), d.size(), C, msg) && msg == c.what, c.what);
    }
    // the order inside a file: keys, indices, len, tags, data
    d[3] = good();
    d[3].data = nullptr;
    d[3].tags = nullptr;
    hb_blocks_check(d.data(), d.size(), C, msg);
    expect(msg == "file 3: tags buffer is NULL", "tags before data");
    d[3].len = 1;
    hb_blocks_check(d.data(), d.size(), C, msg);
    expect(msg.find("file 3: len") == 0, "len before tags");
    d[3].indices = nullptr;
    hb_blocks_check(d.data(), d.size(), C, msg);
    expect(msg == "file 3: indices is NULL", "indices before len");
    d[3].alpha_key = nullptr;
    hb_blocks_check(d.data(), d.size(), C, msg);
    expect(msg == "file 3: a key is NULL", "keys first");
    // the first faulty file wins
    d[1].tags = nullptr;
    hb_blocks_check(d.data(), d.size(), C, msg);
    expect(msg == "file 1: tags buffer is NULL", "the first faulty file");
    // data may be NULL when len == 0
    hb_blocks_desc z = {k1, k2, idx, 1, nullptr, 0, tags};
    expect(hb_blocks_check(&z, 1, C, msg), "one empty block without data");
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
};

// nf files with random lists; the last listed block of a file may be short
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
        for (auto &i : B.idx[f]) i = rnd() % 3 == 0 ? ~0ull - rnd() % 5 : rnd() << (rnd() % 40);
        B.tags[f].assign(nb * tw, 0xee);
        B.d[f] = hb_blocks_desc{B.fk[f].data(), B.ak[f].data(), nb ? B.idx[f].data() : nullptr, nb,
                                len ? B.data[f].data() : nullptr, len, nb ? B.tags[f].data() : nullptr};
    }
}

static void check_plan(const Batch &B, const HbBlkPlan &P, const HbBatchSizes &z, const BlkShape &E, uint64_t cap_blocks,
                       uint64_t cap_bytes) {
    // the segments walk every list once, in order
    size_t s = 0;
    for (uint64_t f = 0; f < B.d.size(); ++f) {
        uint64_t at = 0;
        while (at < B.d[f].nblocks) {
            expect(s < P.segs.size() && P.segs[s].file == f && P.segs[s].first == at && P.segs[s].count >= 1,
                   "segments cover the lists in order", (long long)f, (long long)at);
            if (s >= P.segs.size()) return;
            at += P.segs[s++].count;
        }
        expect(at == B.d[f].nblocks, "a list is covered exactly");
    }
    expect(s == P.segs.size(), "no segment beyond the lists");
    uint64_t seg = 0;
    for (const HbBlkGroup &G : P.groups) {
        expect(G.seg0 == seg && G.nsegs >= 1, "groups partition the segments");
        uint64_t blocks = 0, bytes = 0;
        for (uint64_t k = 0; k < G.nsegs; ++k) {
            const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + k)];
            blocks += X.count;
            bytes += hb_blocks_cost(z, E, hb_blocks_seg_len(B.d[X.file].len, E.C, X.first, X.count), X.count);
        }
        expect(blocks == G.blocks && bytes == G.bytes, "a group's totals");
        expect(G.blocks <= cap_blocks, "the block cap holds", (long long)G.blocks, (long long)cap_blocks);
        expect(G.bytes <= cap_bytes || G.blocks == 1, "the byte cap holds unless one block is alone");
        seg += G.nsegs;
    }
    expect(seg == P.segs.size(), "every segment has a group");
}

static void forced_split() {
    const HbBatchSizes z = sizes<8>();
    const BlkShape E = {310, 10, 32, 4, false, false, false};
    Batch B;
    make_batch(B, 1, E.C, E.tw, 0, 32);
    B.idx[0].assign(10, 5);
    B.data[0].assign(10 * E.C - 3, 1);
    B.tags[0].assign(10 * E.tw, 0);
    B.d[0] = hb_blocks_desc{B.fk[0].data(), B.ak[0].data(), B.idx[0].data(), 10, B.data[0].data(), B.data[0].size(), B.tags[0].data()};
    const HbBlkPlan P = hb_blocks_plan(B.d.data(), 1, z, E, 4, HB_BATCH_BYTES);
    expect(P.groups.size() == 3 && P.segs.size() == 3, "10 blocks under a cap of 4: three groups", (long long)P.groups.size());
    if (P.segs.size() == 3)
        expect(P.segs[0].count == 4 && P.segs[1].count == 4 && P.segs[2].count == 2 && P.segs[2].first == 8, "4 + 4 + 2");
    expect(hb_blocks_seg_len(B.d[0].len, E.C, 8, 2) == 2 * E.C - 3 && hb_blocks_seg_len(B.d[0].len, E.C, 4, 4) == 4 * E.C,
           "a segment's bytes");
    check_plan(B, P, z, E, 4, HB_BATCH_BYTES);
    // two files of 3 under a cap of 4: 3 | 1 + 2 ... a file's list may start in one group and end in the next
    Batch B2;
    make_batch(B2, 2, E.C, E.tw, 0, 32);
    for (int f = 0; f < 2; ++f) {
        B2.idx[f].assign(3, 9);
        B2.data[f].assign(3 * E.C, 2);
        B2.tags[f].assign(3 * E.tw, 0);
        B2.d[f] = hb_blocks_desc{B2.fk[f].data(), B2.ak[f].data(), B2.idx[f].data(), 3, B2.data[f].data(), 3 * E.C, B2.tags[f].data()};
    }
    const HbBlkPlan Q = hb_blocks_plan(B2.d.data(), 2, z, E, 4, HB_BATCH_BYTES);
    expect(Q.groups.size() == 2 && Q.segs.size() == 3 && Q.segs[1].file == 1 && Q.segs[1].count == 1 && Q.segs[2].first == 1,
           "3 + 3 under a cap of 4: (3, 1) (2)");
    // a byte cap below one block's cost: every block alone
    const HbBlkPlan R = hb_blocks_plan(B2.d.data(), 2, z, E, ~0ull, 1);
    expect(R.groups.size() == 6 && R.segs.size() == 6, "a byte cap of 1: six groups of one block");
    check_plan(B2, R, z, E, ~0ull, 1);
}

template <int NL>
static void fills(size_t key_len) {
    const HbBatchSizes z = sizes<NL>();
    const int nr = aes_rounds(key_len);
    uint8_t p_be[NL * 4];
    for (auto &b : p_be) b = (uint8_t)(rnd() | 1);
    p_be[0] |= 0x80;
    for (int round = 0; round < 40; ++round) {
        const uint32_t S = 1 + (uint32_t)(rnd() % 40), ss = NL * 4 - (round % 3 == 0 ? 0 : 1), tw = NL * 4;
        BlkShape E = {(uint64_t)ss * S, S, tw, 1 + (uint32_t)(rnd() % 9), (round & 1) != 0, (round & 2) != 0,
                      ss == 4u * NL && ((uint64_t)ss * S) % 16 == 0};
        Batch B;
        make_batch(B, 1 + rnd() % 7, E.C, tw, 45, key_len);
        const uint64_t cap_blocks = round % 4 == 0 ? 1 + rnd() % 20 : ~0ull;
        const uint64_t cap_bytes = round % 5 == 0 ? 4000 + rnd() % 60000 : HB_BATCH_BYTES;
        const HbBlkPlan P = hb_blocks_plan(B.d.data(), B.d.size(), z, E, cap_blocks, cap_bytes);
        check_plan(B, P, z, E, cap_blocks, cap_bytes);
        PrfParams<NL> P0;
        int n0 = 0;
        expect(make_prf<NL>(B.fk[0].data(), key_len, p_be, sizeof p_be, P0, n0) && n0 == nr, "range template");
        strip(P0);
        uint8_t *const dev = (uint8_t *)(uintptr_t)0x7f0000000000ull + 16 * (rnd() % 8);
        for (const HbBlkGroup &G : P.groups) {
            const HbBlkTotals T = hb_blocks_totals(B.d.data(), P, G, E);
            const HbArena L = hb_blocks_arena(z, E, G, T);
            expect(L.n == 9 && L.total <= G.bytes + 16 * 9, "the arena is inside the group's cost", (long long)L.total,
                   (long long)G.bytes);
            // exactly the uploaded bytes: a write past them is a sanitizer report
            std::vector<uint8_t> host((size_t)L.up_bytes, 0xa5);
            uint64_t bad = ~0ull;
            expect(hb_blocks_fill<NL>(B.d.data(), P, G, E, L, P0, key_len, nr, host.data(), dev, bad), "fill");
            const PrfParams<NL> *hprf = L.at<PrfParams<NL>>(host.data(), HB_BLK_PRF);
            const BatchFile *hf = L.at<BatchFile>(host.data(), HB_BLK_FILES);
            const BatchWaveJob *hj = L.at<BatchWaveJob>(host.data(), HB_BLK_JOBS);
            const BatchMacWg *hw = L.at<BatchMacWg>(host.data(), HB_BLK_WGS);
            const uint64_t *hi = L.at<uint64_t>(host.data(), HB_BLK_IDX);
            uint64_t j = 0, w = 0, fbase = 0, doff = L.off[HB_BLK_DATA], toff = L.off[HB_BLK_TAGS];
            for (uint64_t s = 0; s < G.nsegs; ++s) {
                const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
                const hb_blocks_desc &D = B.d[X.file];
                // schedules: the file's keys under the template's range
                AesKey kf, ka;
                aes_expand(D.f_key, key_len, kf);
                aes_expand(D.alpha_key, key_len, ka);
                expect(memcmp(hprf[2 * s].rk, kf.rk, 16 * (size_t)(nr + 1)) == 0 &&
                           memcmp(hprf[2 * s + 1].rk, ka.rk, 16 * (size_t)(nr + 1)) == 0,
                       "key schedules: f_key then alpha_key");
                expect(memcmp(hprf[2 * s].R, P0.R, sizeof P0.R) == 0 && hprf[2 * s + 1].nb == P0.nb &&
                           hprf[2 * s].topmask == P0.topmask,
                       "the schedules keep the template's range");
                // the record
                const uint64_t slen = hb_blocks_seg_len(D.len, E.C, X.first, X.count);
                const BatchFile &F = hf[s];
                expect(F.len == slen && F.nblocks == X.count && F.fbase == fbase, "record: len, nblocks, fbase");
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
                expect(((F.flags & HB_BF_LOAD16) != 0) == (E.shape16 && (uintptr_t)F.data % 16 == 0), "load16");
                expect(((F.flags & HB_BF_TAGS4) != 0) == ((uintptr_t)F.tags % 4 == 0), "tags4");
                // indices
                expect(memcmp(hi + fbase, D.indices + X.first, (size_t)X.count * 8) == 0, "indices: the segment's slice");
                // wave-jobs: alpha in 16s, then F in 16s
                for (uint64_t b = 0; b < S; b += 16, ++j)
                    expect(hj[j].file == s && hj[j].kind == 1 && hj[j].first == b && hj[j].count == (S - b < 16 ? S - b : 16),
                           "alpha wave-jobs");
                for (uint64_t b = 0; b < X.count; b += 16, ++j)
                    expect(hj[j].file == s && hj[j].kind == 0 && hj[j].first == b &&
                               hj[j].count == (X.count - b < 16 ? X.count - b : 16),
                           "F wave-jobs");
                for (uint64_t b = 0; b < X.count; b += E.bpw, ++w)
                    expect(hw[w].file == s && hw[w].first == b, "MAC workgroups");
                fbase += X.count;
            }
            expect(j == T.nj && w == T.nwg && fbase == G.blocks, "the tables add up");
            expect(E.data_dev || doff == L.off[HB_BLK_DATA] + T.dbytes, "the data cursor ends at the section's end");
            expect(doff <= L.up_bytes, "the data ends inside the upload");
            // the tags' way back: the download starts at the tags section
            if (!E.tags_dev) {
                std::vector<uint8_t> down((size_t)T.tbytes);
                for (size_t k = 0; k < down.size(); ++k) down[k] = (uint8_t)(k * 7 + 1);
                hb_blocks_tags_out(B.d.data(), P, G, E, down.data());
                uint64_t off = 0;
                for (uint64_t s = 0; s < G.nsegs; ++s) {
                    const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
                    expect(memcmp(B.tags[X.file].data() + X.first * tw, down.data() + off, (size_t)(X.count * tw)) == 0,
                           "tags back at the segment's place");
                    off += hb_up16(X.count * tw);
                }
            }
        }
        // a key the expansion rejects is reported with its file
        if (!P.groups.empty() && round == 0) {
            const HbBlkGroup &G = P.groups[0];
            const HbBlkTotals T = hb_blocks_totals(B.d.data(), P, G, E);
            const HbArena L = hb_blocks_arena(z, E, G, T);
            std::vector<uint8_t> host((size_t)L.up_bytes);
            uint64_t bad = ~0ull;
            expect(!hb_blocks_fill<NL>(B.d.data(), P, G, E, L, P0, key_len, nr == 10 ? 12 : 10, host.data(), dev, bad) &&
                       bad == P.segs[(size_t)G.seg0].file,
                   "a key of another round count");
        }
    }
}

int main() {
    len_bounds();
    check_order();
    forced_split();
    fills<8>(32);
    fills<8>(16);
    fills<32>(24);
    fills<64>(32);
    if (g_bad) {
        printf("%d of %d checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
