// hb_emixed_host.hpp -- what the mixed-owner encodes (hb_encode_mixed,
// hb_cxx_encode_mixed) decide on the host before any HIP call, beyond what they
// share with the other batches (hb_batch_host.hpp, hb_mixed_host.hpp: the class
// partition, the prefix sums, the conversion pass's workgroup table, the prime
// cache): a group's arena layout and a file's cost in it, the F-buffer bases,
// the PySwizzle side's wave-job table and the MAC launch's workgroup table with
// a sector count per file.  Pure host code: no HIP, no context, so that a
// stand-alone program can walk it (tests/emixed_host/host_main.cpp, built with
// AddressSanitizer and UBSan).
#pragma once
#include <vector>

#include "hb_mixed_host.hpp"

// ------------------------------------------------------------------ tables
// The MAC launches of a group, one per shape.  A file of 2 <= S <= T sectors
// takes the split shape (hb_emixed_mac_split_kernel: T = HbMacSplit<NL>::T
// threads per workgroup whatever S is, lane (k, j) sector j of block k, T / S
// blocks per workgroup); S = 1 or S > T the lane-per-block shape
// (hb_emixed_mac_lane_kernel: 256 blocks per workgroup).
#define HB_EM_LANE_BLOCKS 256u
inline bool hb_em_split(uint32_t T, uint64_t S) { return S >= 2 && S <= T; }
inline uint32_t hb_em_bpw(uint32_t T, uint64_t S) { return hb_em_split(T, S) ? (uint32_t)(T / S) : HB_EM_LANE_BLOCKS; }
inline uint64_t hb_em_mac_wg_count(uint32_t T, uint64_t S, uint64_t mac_blocks) {
    const uint64_t bpw = hb_em_bpw(T, S);
    return (mac_blocks + bpw - 1) / bpw;
}

// The device reads an entry as two dwords (BatchMacWg, hb_args.hpp): blocks
// [first, first + hb_em_bpw(T, S[file])) of one file.  mac_blocks[f]: the
// file's blocks that the MAC launches tag (cxx: those that read a sector).
// One table for both launches: the split shape's workgroups first (*nsplit of
// them), the lane-per-block shape's behind them; the result is the sum.
struct HbEmWg {
    uint32_t file, first;
};
#define HB_EMWG_BYTES 8u
inline uint64_t hb_em_mac_wgs(const uint32_t *S, const uint64_t *mac_blocks, uint64_t n, uint32_t T, HbEmWg *out,
                              uint64_t *nsplit) {
    uint64_t w = 0;
    for (int lane = 0; lane < 2; ++lane) {
        for (uint64_t f = 0; f < n; ++f) {
            if (hb_em_split(T, S[f]) == (lane != 0)) continue;
            const uint32_t bpw = hb_em_bpw(T, S[f]);
            for (uint64_t b = 0; b < mac_blocks[f]; b += bpw, ++w)
                if (out) out[w] = HbEmWg{(uint32_t)f, (uint32_t)b};
        }
        if (!lane && nsplit) *nsplit = w;
    }
    return w;
}

// The PySwizzle side's queue (BatchWaveJob, hb_args.hpp: four dwords): up to 16
// evaluations of one file under one key; a file's ceil(S / 16) alpha wave-jobs
// (kind 1) directly before its F wave-jobs (kind 0), as hb_encode_many queues
// them.  (The cxx side's queue is the planner's: hb_cbatch_jobs.)
struct HbEmJob {
    uint32_t file, kind, first, count;
};
inline uint64_t hb_em_job_count(uint64_t S, uint64_t blocks) { return (S + 15) / 16 + (blocks + 15) / 16; }
inline uint64_t hb_em_jobs(const uint32_t *S, const uint64_t *blocks, uint64_t n, HbEmJob *out) {
    uint64_t j = 0;
    for (uint64_t f = 0; f < n; ++f)
        for (uint32_t kind = 1; kind != ~0u; --kind) {
            const uint64_t cnt = kind ? (uint64_t)S[f] : blocks[f];
            for (uint64_t a = 0; a < cnt; a += 16, ++j)
                if (out) out[j] = HbEmJob{(uint32_t)f, kind, (uint32_t)a, (uint32_t)(cnt - a < 16 ? cnt - a : 16)};
        }
    return j;
}

// first[f] = the file's first block in the group's F buffer; the result is the
// group's block count (the alpha slots: hb_mixed_prefix with add = 0)
inline uint64_t hb_em_fbases(const uint64_t *blocks, uint64_t n, std::vector<uint64_t> &first) {
    first.resize((size_t)n);
    uint64_t at = 0;
    for (uint64_t f = 0; f < n; ++f) {
        first[(size_t)f] = at;
        at += blocks[f];
    }
    return at;
}

// ------------------------------------------------------------------ arena layout
// hb_encode_mixed and hb_cxx_encode_mixed:
//     [prf | files | records | slot ranges | wave-jobs | MAC workgroups | conversion workgroups | host files] (uploaded)
//     [F | alpha | tags]
// nf files of `blocks` blocks and `slots` alpha slots in all, nj wave-jobs, nwg
// MAC workgroups, nmwg conversion workgroups, dbytes / tbytes of host-resident
// files / host-bound tags (each file's rounded up to 16).  rec: sizeof(MxRec<NL>).
// The slot ranges are the conversion pass's per-file entries (z.pproof: PbProof
// with obase = the file's first alpha slot and chunks = S).
enum { HB_EMX_PRF, HB_EMX_FILES, HB_EMX_RECS, HB_EMX_SLOTS, HB_EMX_JOBS, HB_EMX_WGS, HB_EMX_MONTWG, HB_EMX_DATA,
       HB_EMX_FV, HB_EMX_AM, HB_EMX_TAGS, HB_EMX_SECTIONS };
inline HbArena hb_em_arena(const HbBatchSizes &z, uint64_t rec, uint64_t nf, uint64_t nj, uint64_t nwg, uint64_t nmwg,
                           uint64_t dbytes, uint64_t blocks, uint64_t slots, uint64_t tbytes) {
    HbArena L;
    L.add(2 * nf * z.prf);
    L.add(nf * z.file);
    L.add(nf * rec);
    L.add(nf * z.pproof);
    L.add(nj * HB_JOB_BYTES);
    L.add(nwg * HB_EMWG_BYTES);
    L.add(nmwg * HB_MXWG_BYTES);
    L.add(dbytes);
    L.end_upload();
    L.add(blocks * z.limbs);
    L.add(slots * z.limbs);
    L.add(tbytes);
    return L;
}
// scratch bytes of one file of nb blocks and S sectors with nj wave-jobs and nwg
// MAC workgroups (exact; the section padding is the arena's: at most 16 per
// section)
inline uint64_t hb_em_cost(const HbBatchSizes &z, uint64_t rec, uint64_t nj, uint64_t nwg, uint64_t data_up, uint64_t nb,
                           uint64_t S, uint64_t tags_up) {
    return 2 * z.prf + z.file + rec + z.pproof + nj * HB_JOB_BYTES + nwg * HB_EMWG_BYTES +
           hb_mixed_mont_wg_count(S) * HB_MXWG_BYTES + data_up + nb * z.limbs + S * z.limbs + tags_up;
}
