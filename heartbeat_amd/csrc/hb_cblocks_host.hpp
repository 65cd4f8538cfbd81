// hb_cblocks_host.hpp -- what hb_cxx_encode_blocks_many decides and writes on
// the host before any HIP call: the descriptor and index-range checks, the
// split of the files' block lists into segments and groups with each group's
// queue of wave-jobs, a group's arena layout, and the fill of its staging
// buffer -- key schedules, file records, wave-jobs, MAC workgroups, the
// narrowed index table and the host-resident blocks.  Pure host code: no HIP,
// no context; a stand-alone program walks it under ASan and UBSan
// (tests/cblocks_emul/main.cpp).
//
// Segments and groups are hb_blocks_host.hpp's (HbBlkSeg, HbBlkGroup: a
// segment is a file of the batch to the kernels, a long list continues as
// another segment in the next group), the descriptor checks are
// hb_blocks_check, the wave-jobs are the cxx batch's (HbCbJob, sorted by
// hb_cbatch_jobs).  What is the cxx call's own:
//   - an index is the cxx prf's unsigned int: 2^32 and above is refused, and
//     the device table holds u32;
//   - wave-jobs are HB_CB_JOB evaluations wide, longest first per group;
//   - a list's last block that is empty reads no sector and keeps F unreduced
//     (hb_cbatch_args.hpp).  It belongs to the list's last segment alone; that
//     segment's BatchFile::nblocks -- the MAC's count -- is one less than its
//     F evaluations, and it gets MAC workgroups for the smaller count.
#pragma once
#include "hb_blocks_host.hpp"

namespace hbhost {

// The call's checks that need no GPU, in order; the result is 0, HB_EINVAL or
// HB_EUNSUPPORTED with `msg` naming the file:
//   1. every descriptor (hb_blocks_check: per file keys, indices, len, tags,
//      data; the first fault of the first faulty file): HB_EINVAL;
//   2. every index, file by file, list position by list position: the first
//      one of 2^32 or above is HB_EUNSUPPORTED.
// A bad descriptor in a later file therefore wins over a wide index in an
// earlier one.
inline int hb_cblocks_check(const hb_blocks_desc *files, u64 nfiles, u64 C, std::string &msg) {
    if (!hb_blocks_check(files, nfiles, C, msg)) return HB_EINVAL;
    for (u64 i = 0; i < nfiles; ++i)
        for (u64 k = 0; k < files[i].nblocks; ++k)
            if (files[i].indices[k] >> 32) {
                msg = "file " + std::to_string(i) + ": index " + std::to_string(files[i].indices[k]) + " (listed block " +
                      std::to_string(k) + ") does not fit the cxx prf's unsigned int";
                return HB_EUNSUPPORTED;
            }
    return 0;
}

// blocks of a segment of seg_len bytes that read a sector: all of its `count`
// blocks unless the last one is empty
inline u64 hb_cblocks_mac(u64 seg_len, u64 C, u64 count) { return seg_len > (count - 1) * C ? count : count - 1; }
inline u64 hb_cblocks_jobs(const BlkShape &E, u64 count) {
    return ((u64)E.S + HB_CB_JOB - 1) / HB_CB_JOB + (count + HB_CB_JOB - 1) / HB_CB_JOB;
}

// scratch bytes of one segment inside a group (hb_cblocks_arena's sections, no slack)
inline u64 hb_cblocks_cost(const HbBatchSizes &z, const BlkShape &E, u64 seg_len, u64 count) {
    return 2 * z.prf + z.file + hb_cblocks_jobs(E, count) * HB_JOB_BYTES + hb_blocks_wgs(E, hb_cblocks_mac(seg_len, E.C, count)) * z.wg +
           count * 4 + hb_blocks_data_up(E, seg_len) + count * z.limbs + (u64)E.S * z.limbs + hb_blocks_tags_up(E, count);
}

struct HbCblkPlan {
    HbBlkPlan blk;            // segments and groups (hb_blocks_plan_by under hb_cblocks_cost)
    HbCbPlan cb;              // cb.groups[g] = blk.groups[g]: its wave-jobs cb.jobs[job0, job0 + njobs), item = segment in the group
};

inline HbCblkPlan hb_cblocks_plan(const hb_blocks_desc *files, u64 nfiles, const HbBatchSizes &z, const BlkShape &E,
                                  u64 cap_blocks, u64 cap_bytes) {
    HbCblkPlan P;
    P.blk = hb_blocks_plan_by(files, nfiles, cap_blocks, cap_bytes, [&](u64 i, u64 first, u64 n) {
        return hb_cblocks_cost(z, E, hb_blocks_seg_len(files[i].len, E.C, first, n), n);
    });
    // the cxx batch's queue builder over the segments as items
    std::vector<HbCbItemReq> req(P.blk.segs.size());
    for (size_t s = 0; s < req.size(); ++s) {
        req[s] = HbCbItemReq{};
        req[s].n[HB_CB_F] = P.blk.segs[s].count;
        req[s].n[HB_CB_ALPHA] = E.S;
        req[s].aes[HB_CB_F] = req[s].aes[HB_CB_ALPHA] = E.tw / 16;
        P.cb.order.push_back(s);
    }
    for (const HbBlkGroup &G : P.blk.groups) P.cb.groups.push_back(HbCbGroup{G.seg0, G.nsegs, 0, 0, G.blocks, G.bytes});
    hb_cbatch_jobs(req.data(), P.cb);
    return P;
}

// hb_cxx_encode_blocks_many:
//     [prf | files | jobs | wgs | indices (u32) | host blocks] (uploaded) [F | alpha | tags]
enum { HB_CBK_PRF, HB_CBK_FILES, HB_CBK_JOBS, HB_CBK_WGS, HB_CBK_IDX, HB_CBK_DATA, HB_CBK_FV, HB_CBK_AM, HB_CBK_TAGS };

// nj: the group's wave-jobs (its HbCbGroup::njobs)
inline HbBlkTotals hb_cblocks_totals(const hb_blocks_desc *files, const HbBlkPlan &P, const HbBlkGroup &G, const BlkShape &E,
                                     u64 nj) {
    HbBlkTotals T;
    T.nj = nj;
    for (u64 s = 0; s < G.nsegs; ++s) {
        const HbBlkSeg &X = P.segs[(size_t)(G.seg0 + s)];
        const u64 slen = hb_blocks_seg_len(files[X.file].len, E.C, X.first, X.count);
        T.nwg += hb_blocks_wgs(E, hb_cblocks_mac(slen, E.C, X.count));
        T.dbytes += hb_blocks_data_up(E, slen);
        T.tbytes += hb_blocks_tags_up(E, X.count);
    }
    return T;
}
inline HbArena hb_cblocks_arena(const HbBatchSizes &z, const BlkShape &E, const HbBlkGroup &G, const HbBlkTotals &T) {
    HbArena L;
    L.add(2 * G.nsegs * z.prf);
    L.add(G.nsegs * z.file);
    L.add(T.nj * HB_JOB_BYTES);
    L.add(T.nwg * z.wg);
    L.add(G.blocks * 4);
    L.add(T.dbytes);
    L.end_upload();
    L.add(G.blocks * z.limbs);
    L.add(G.nsegs * (u64)E.S * z.limbs);
    L.add(T.tbytes);
    return L;
}

// The uploaded sections of group g into `host` (the staging mirror of the
// arena at device address `dev`).  Segment s of the group is item s of the
// launches.  The indices have passed hb_cblocks_check: narrowing loses nothing.
// False: a key the AES expansion rejects (bad_file: its descriptor).
template <int NL>
bool hb_cblocks_fill(const hb_blocks_desc *files, const HbCblkPlan &P, size_t g, const BlkShape &E, const HbArena &L,
                     const PrfParams<NL> &P0, size_t key_len, int nr, uint8_t *host, uint8_t *dev, u64 &bad_file) {
    const HbBlkGroup &G = P.blk.groups[g];
    const HbCbGroup &Q = P.cb.groups[g];
    PrfParams<NL> *hprf = L.at<PrfParams<NL>>(host, HB_CBK_PRF);
    BatchFile *hfiles = L.at<BatchFile>(host, HB_CBK_FILES);
    BatchMacWg *hwgs = L.at<BatchMacWg>(host, HB_CBK_WGS);
    u32 *hidx = L.at<u32>(host, HB_CBK_IDX);
    u64 doff = L.off[HB_CBK_DATA], toff = L.off[HB_CBK_TAGS], w = 0, fbase = 0;
    for (u64 s = 0; s < G.nsegs; ++s) {
        const HbBlkSeg &X = P.blk.segs[(size_t)(G.seg0 + s)];
        const hb_blocks_desc &D = files[X.file];
        if (!schedule<NL>(P0, D.f_key, key_len, nr, hprf[2 * s + HB_CB_F]) ||
            !schedule<NL>(P0, D.alpha_key, key_len, nr, hprf[2 * s + HB_CB_ALPHA])) {
            bad_file = X.file;
            return false;
        }
        const u64 slen = hb_blocks_seg_len(D.len, E.C, X.first, X.count);
        const u64 mac = hb_cblocks_mac(slen, E.C, X.count);
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
        F.nblocks = (u32)mac;
        F.flags = (E.shape16 && (uintptr_t)F.data % 16 == 0 ? HB_BF_LOAD16 : 0u) | ((uintptr_t)F.tags % 4 == 0 ? HB_BF_TAGS4 : 0u);
        for (u64 k = 0; k < X.count; ++k) hidx[fbase + k] = (u32)D.indices[X.first + k];
        for (u64 b = 0; b < mac; b += E.bpw) hwgs[w++] = BatchMacWg{(u32)s, (u32)b};
        fbase += X.count;
    }
    if (Q.njobs) memcpy(host + L.off[HB_CBK_JOBS], P.cb.jobs.data() + Q.job0, (size_t)(Q.njobs * sizeof(HbCbJob)));
    return true;
}

}  // namespace hbhost
