// hb_blocks_host.hpp -- what hb_encode_blocks_many decides and writes on the
// host before any HIP call: the descriptor checks, the split of the files'
// block lists into segments and groups, a group's arena layout, and the fill
// of its staging buffer -- key schedules, file records, wave-jobs, MAC
// workgroups, the index table and the host-resident blocks.  Pure host code:
// no HIP, no context; a stand-alone program walks it under ASan and UBSan
// (tests/blocks_emul/main.cpp).
//
// A segment is a run [first, first + count) of one file's list.  To the
// kernels it is a file of the batch: its own pair of key schedules, its own
// alpha table, a BatchFile whose data are the run's packed blocks and whose
// fbase is the run's place in the group's index table and F buffer.  A list
// that does not fit a group continues as another segment in the next group
// (alpha is drawn again there: S evaluations against a group's worth of
// blocks).  An empty list has no segment.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "hb_pv_host.hpp"   // schedule(), push_jobs16(), stage_in(); with it hb_batch_host.hpp, hb_args.hpp

namespace hbhost {

struct BlkShape {
    u64 C;                    // block size, sectors * ss
    u32 S, tw, bpw;           // sectors, tag width, blocks per MAC workgroup (hb_batch_mac_bpw)
    bool data_dev, tags_dev;
    bool shape16;             // ss and C allow the 16-byte sector loads (the data address decides the rest)
};

// A file's byte count must lie in [(nblocks - 1) C, nblocks C]: only the last
// listed block may be short.  nblocks == 0 allows len == 0 alone.
inline bool hb_blocks_len_ok(u64 nblocks, u64 len, u64 C) {
    if (nblocks == 0) return len == 0;
    if (nblocks - 1 > ~0ull / C) return false;              // (nblocks - 1) C does not fit: no len can reach it
    if (len < (nblocks - 1) * C) return false;
    return nblocks > ~0ull / C || len <= nblocks * C;       // nblocks C past 2^64: every len is below it
}

// Every descriptor, in order, before any GPU work; the first fault of the
// first faulty file wins.  Per file: keys, indices, len, tags, data.
inline bool hb_blocks_check(const hb_blocks_desc *files, u64 nfiles, u64 C, std::string &msg) {
    for (u64 i = 0; i < nfiles; ++i) {
        const hb_blocks_desc &D = files[i];
        const char *what = nullptr;
        if (!D.f_key || !D.alpha_key) what = "a key is NULL";
        else if (!D.indices && D.nblocks) what = "indices is NULL";
        else if (!hb_blocks_len_ok(D.nblocks, D.len, C)) what = "len is outside [(nblocks - 1) * C, nblocks * C]";
        else if (!D.tags && D.nblocks) what = "tags buffer is NULL";
        else if (!D.data && D.len) what = "data buffer is NULL";
        if (what) {
            msg = "file " + std::to_string(i) + ": " + what;
            return false;
        }
    }
    return true;
}

struct HbBlkSeg {
    u64 file;                 // position of the descriptor in the call
    u64 first, count;         // listed blocks [first, first + count), count >= 1
};
struct HbBlkGroup {
    u64 seg0, nsegs;          // segs[seg0, seg0 + nsegs)
    u64 blocks, bytes;        // listed blocks and scratch bytes of the group
};
struct HbBlkPlan {
    std::vector<HbBlkSeg> segs;
    std::vector<HbBlkGroup> groups;
};

// most listed blocks in one segment: BatchFile.nblocks and a wave-job's first are 32-bit
#define HB_BLK_SEG_MAX (1ull << 31)

// bytes of blocks [first, first + count) of a list of `len` bytes
inline u64 hb_blocks_seg_len(u64 len, u64 C, u64 first, u64 count) {
    const u64 a = first * C;                       // first < nblocks: inside len's bounds
    const u64 left = len - a;
    return count <= left / C ? count * C : left;
}
inline u64 hb_blocks_jobs(const BlkShape &E, u64 count) { return ((u64)E.S + 15) / 16 + (count + 15) / 16; }
inline u64 hb_blocks_wgs(const BlkShape &E, u64 count) { return (count + E.bpw - 1) / E.bpw; }
inline u64 hb_blocks_data_up(const BlkShape &E, u64 seg_len) { return E.data_dev ? 0 : hb_up16(seg_len); }
inline u64 hb_blocks_tags_up(const BlkShape &E, u64 count) { return E.tags_dev ? 0 : hb_up16(count * E.tw); }

// scratch bytes of one segment inside a group (hb_blocks_arena's sections, no slack)
inline u64 hb_blocks_cost(const HbBatchSizes &z, const BlkShape &E, u64 seg_len, u64 count) {
    return 2 * z.prf + z.file + hb_blocks_jobs(E, count) * HB_JOB_BYTES + hb_blocks_wgs(E, count) * z.wg + count * 8 +
           hb_blocks_data_up(E, seg_len) + count * z.limbs + (u64)E.S * z.limbs + hb_blocks_tags_up(E, count);
}

// Segments and groups, in the caller's order.  A group ends before the block
// that would take it over cap_blocks listed blocks or cap_bytes of scratch; a
// single block alone may pass cap_bytes (every block gets a group).
// seg_cost(file, first, n): scratch bytes of blocks [first, first + n) of that
// file's list as one segment, growing with n (hb_blocks_cost here;
// hb_cblocks_host.hpp has the cxx call's).
template <class Cost>
HbBlkPlan hb_blocks_plan_by(const hb_blocks_desc *files, u64 nfiles, u64 cap_blocks, u64 cap_bytes, Cost &&seg_cost) {
    HbBlkPlan P;
    if (cap_blocks < 1) cap_blocks = 1;
    HbBlkGroup G = {0, 0, 0, 0};
    auto close = [&]() {
        if (G.nsegs) P.groups.push_back(G);
        G = HbBlkGroup{P.segs.size(), 0, 0, 0};
    };
    for (u64 i = 0; i < nfiles; ++i) {
        u64 first = 0;
        while (first < files[i].nblocks) {
            const u64 left = files[i].nblocks - first;
            u64 room = cap_blocks - G.blocks;
            if (room > left) room = left;
            if (room > HB_BLK_SEG_MAX) room = HB_BLK_SEG_MAX;
            const u64 bytes_left = cap_bytes > G.bytes ? cap_bytes - G.bytes : 0;
            auto cost = [&](u64 n) { return seg_cost(i, first, n); };
            // the most blocks whose segment still fits: the cost grows with the count
            u64 lo = 0, hi = room;
            while (lo < hi) {
                const u64 mid = lo + (hi - lo + 1) / 2;
                if (cost(mid) <= bytes_left) lo = mid;
                else hi = mid - 1;
            }
            if (lo == 0) {
                if (G.nsegs) {
                    close();
                    continue;
                }
                lo = 1;   // alone in its group
            }
            P.segs.push_back(HbBlkSeg{i, first, lo});
            ++G.nsegs;
            G.blocks += lo;
            G.bytes += cost(lo);
            first += lo;
            if (G.blocks >= cap_blocks) close();
        }
    }
    close();
    return P;
}
inline HbBlkPlan hb_blocks_plan(const hb_blocks_desc *files, u64 nfiles, const HbBatchSizes &z, const BlkShape &E,
                                u64 cap_blocks, u64 cap_bytes) {
    return hb_blocks_plan_by(files, nfiles, cap_blocks, cap_bytes, [&](u64 i, u64 first, u64 n) {
        return hb_blocks_cost(z, E, hb_blocks_seg_len(files[i].len, E.C, first, n), n);
    });
}

// hb_encode_blocks_many:
//     [prf | files | jobs | wgs | indices | host blocks] (uploaded) [F | alpha | tags]
enum { HB_BLK_PRF, HB_BLK_FILES, HB_BLK_JOBS, HB_BLK_WGS, HB_BLK_IDX, HB_BLK_DATA, HB_BLK_FV, HB_BLK_AM, HB_BLK_TAGS };

struct HbBlkTotals {
    u64 nj = 0, nwg = 0, dbytes = 0, tbytes = 0;
};
inline HbBlkTotals hb_blocks_totals(const hb_blocks_desc *files, const HbBlkPlan &P, const HbBlkGroup &G, const BlkShape &E) {
    HbBlkTotals T;
    for (u64 s = 0; s < G.nsegs; ++s) {
        const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
        T.nj += hb_blocks_jobs(E, X.count);
        T.nwg += hb_blocks_wgs(E, X.count);
        T.dbytes += hb_blocks_data_up(E, hb_blocks_seg_len(files[X.file].len, E.C, X.first, X.count));
        T.tbytes += hb_blocks_tags_up(E, X.count);
    }
    return T;
}
inline HbArena hb_blocks_arena(const HbBatchSizes &z, const BlkShape &E, const HbBlkGroup &G, const HbBlkTotals &T) {
    HbArena L;
    L.add(2 * G.nsegs * z.prf);
    L.add(G.nsegs * z.file);
    L.add(T.nj * HB_JOB_BYTES);
    L.add(T.nwg * z.wg);
    L.add(G.blocks * 8);
    L.add(T.dbytes);
    L.end_upload();
    L.add(G.blocks * z.limbs);
    L.add(G.nsegs * (u64)E.S * z.limbs);
    L.add(T.tbytes);
    return L;
}

// The uploaded sections of one group into `host` (the staging mirror of the
// arena at device address `dev`).  Segment s of the group is file s of the
// launches; its alpha wave-jobs come directly before its F wave-jobs, as the
// batched encode queues them.  False: a key the AES expansion rejects
// (bad_file: its descriptor).
template <int NL>
bool hb_blocks_fill(const hb_blocks_desc *files, const HbBlkPlan &P, const HbBlkGroup &G, const BlkShape &E, const HbArena &L,
                    const PrfParams<NL> &P0, size_t key_len, int nr, uint8_t *host, uint8_t *dev, u64 &bad_file) {
    PrfParams<NL> *hprf = L.at<PrfParams<NL>>(host, HB_BLK_PRF);
    BatchFile *hfiles = L.at<BatchFile>(host, HB_BLK_FILES);
    BatchWaveJob *hjobs = L.at<BatchWaveJob>(host, HB_BLK_JOBS);
    BatchMacWg *hwgs = L.at<BatchMacWg>(host, HB_BLK_WGS);
    u64 *hidx = L.at<u64>(host, HB_BLK_IDX);
    u64 doff = L.off[HB_BLK_DATA], toff = L.off[HB_BLK_TAGS], j = 0, w = 0, fbase = 0;
    for (u64 s = 0; s < G.nsegs; ++s) {
        const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
        const hb_blocks_desc &D = files[X.file];
        if (!schedule<NL>(P0, D.f_key, key_len, nr, hprf[2 * s]) || !schedule<NL>(P0, D.alpha_key, key_len, nr, hprf[2 * s + 1])) {
            bad_file = X.file;
            return false;
        }
        const u64 slen = hb_blocks_seg_len(D.len, E.C, X.first, X.count);
        BatchFile &F = hfiles[s];
        memset(&F, 0, sizeof F);
        F.data = stage_in(E.data_dev, D.data ? D.data + X.first * E.C : nullptr, slen, host, dev, doff);
        F.len = slen;
        F.tags = D.tags + X.first * E.tw;
        if (!E.tags_dev) {
            F.tags = dev + toff;
            toff += hb_blocks_tags_up(E, X.count);
        }
        F.fbase = fbase;
        F.nblocks = (u32)X.count;
        F.flags = (E.shape16 && (uintptr_t)F.data % 16 == 0 ? HB_BF_LOAD16 : 0u) | ((uintptr_t)F.tags % 4 == 0 ? HB_BF_TAGS4 : 0u);
        memcpy(hidx + fbase, D.indices + X.first, (size_t)X.count * 8);
        push_jobs16(hjobs, j, s, 1u, E.S);
        push_jobs16(hjobs, j, s, 0u, X.count);
        for (u64 b = 0; b < X.count; b += E.bpw) hwgs[w++] = BatchMacWg{(u32)s, (u32)b};
        fbase += X.count;
    }
    return true;
}

// Host-bound tags of one group back out of the download (`host`: its head)
inline void hb_blocks_tags_out(const hb_blocks_desc *files, const HbBlkPlan &P, const HbBlkGroup &G, const BlkShape &E,
                               const uint8_t *host) {
    u64 off = 0;
    for (u64 s = 0; s < G.nsegs; ++s) {
        const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
        memcpy(files[X.file].tags + X.first * E.tw, host + off, (size_t)(X.count * E.tw));
        off += hb_blocks_tags_up(E, X.count);
    }
}

}  // namespace hbhost
