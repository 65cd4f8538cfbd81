// hb_onehash_host.hpp -- host side of hb_onehash_generate_many,
// hb_onehash_meet_many, hb_onehash_pick_blocks_many and
// hb_onehash_generate_drawn_many (pure C++, no HIP calls): the descriptor
// checks, the per-file tables the kernels index, the host seed chain, which
// host files are uploaded whole and which are gathered, and the gather itself.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/hbswizzle.h"
#include "hb_onehash_args.hpp"

namespace hbhost {

// Jobs from which a call is worth the GPU: below, heartbeat_amd.OneHash stays
// on its host path (hb_onehash_device_min_jobs).  One 1 MiB file on disk,
// forced host path against forced GPU path, min .. max ms of 7 calls
// (profiles/many/onehash_rate.json, "crossover_jobs"):
//   jobs   meet host      meet GPU       generate host   generate GPU
//     64   0.124..0.126   0.237..0.254   0.166..0.244    0.252..0.295
//    128   0.245..0.249   0.274..0.290   0.321..0.339    0.299..0.338
//    256   0.487..0.492   0.351..0.369   0.633..0.662    0.382..0.391
//    512   0.982..1.013   0.486..0.501   1.271..1.327    0.556..0.569
// The host pays 1.9 us a job, the GPU 0.2 ms a call and 0.55 us a job: the
// lines cross near 150 jobs, and 256 is the first measured count at which the
// GPU's slowest call beats the host's fastest, for both calls.
const uint64_t OH_DEVICE_MIN_JOBS = 256;

// Files from which the device chain beats the host's.  One lane walks a
// file's chain whatever the batch, so the device costs a constant (1000
// links: 2.7 ms) where the host pays per file (0.16 ms each).
// generate_challenges_many of small device-resident files x 1000, fastest of
// 7 calls in ms, host chain against device chain: 1 file 0.85 / 3.51,
// 4 files 2.91 / 5.21, 16 files 11.49 / 12.16, 64 files 52.6 / 45.3,
// 256 files 249 / 218 (profiles/many/onehash_rate.json, "chain").  The
// difference falls by 0.164 ms a file between 16 and 64 files and crosses
// zero at 20.  The calls' slowest rounds (30 ms and more above the fastest,
// in both arms) hide the difference: no row has the device's slowest under
// the host's fastest.
const uint64_t OH_CHAIN_DEVICE_MIN_FILES = 20;

// Jobs from which a GPU generate call of one file draws its positions on the
// device when the caller does not say (hb_onehash_draw_device_min_jobs).
// generate_challenges on one 1 MiB file, GPU path forced, the parent commit's
// tree (pick_blocks in Python) against this one with draw="device", min .. max
// ms of 5 alternating rounds (profiles/many/onehash_draw_rate.json, "sweep"):
//   jobs   parent, disk    device draw, disk   parent, resident   device draw, resident
//    256   0.434..0.526    0.488..0.505        0.318..0.328       0.424..0.434
//    512   0.579..0.612    0.598..0.695        0.479..0.509       0.529..0.540
//   1024   0.945..0.962    0.830..0.840        0.845..0.861       0.760..0.775
//   4096   3.051..3.394    2.133..2.295        2.957..3.009       1.996..2.098
// The draw launch costs 0.1 ms a call (one lane seeds the state) and saves
// 0.25 us a job: 1024 is the first measured count at which the device draw's
// slowest round beats the parent's fastest, from disk and resident.  Calls of
// several files stay opt-in: 256 files x 1000 measured 196..242 against
// 238..272 ms from disk and 159..221 against 195..263 resident, lower at both
// ends but with the slowest round above the parent's fastest.
const uint64_t OH_DRAW_DEVICE_MIN_JOBS = 1024;

// A host file is uploaded whole up to this many bytes, the Merkle scheme's
// threshold; above it only the jobs' segments go to the device.
inline uint64_t oh_upload_max(uint64_t jobs) {
    const uint64_t floor = 8ull << 20;
    if (jobs > (~0ull / 2) / HB_ONEHASH_CHUNK) return ~0ull;
    const uint64_t twice = 2 * jobs * HB_ONEHASH_CHUNK;
    return twice > floor ? twice : floor;
}

struct OhPlan {
    std::vector<OhFile> files;
    uint64_t jobs = 0;
};

inline void oh_words(const uint8_t *b, u32 w[8]) {
    for (int t = 0; t < 8; ++t)
        w[t] = ((u32)b[4 * t] << 24) | ((u32)b[4 * t + 1] << 16) | ((u32)b[4 * t + 2] << 8) | b[4 * t + 3];
}

inline void oh_bytes(const u32 w[8], uint8_t *b) {
    for (int t = 0; t < 8; ++t)
        for (int k = 0; k < 4; ++k) b[4 * t + k] = (uint8_t)(w[t] >> (24 - 8 * k));
}

inline bool oh_block_ok(uint64_t block, uint64_t len) { return block < len; }

// The generate side's descriptors, hb_onehash_gen_desc or
// hb_onehash_drawn_desc: check every one and fill the table (data pointers
// are the runtime's).  positions(i, who, code, err) checks where file i's
// blocks come from.  code / err as the C ABI reports them.
template <class Desc, class Positions>
inline bool oh_plan_files(const Desc *d, uint64_t nfiles, const uint8_t *seeds_out, const uint8_t *responses_out,
                          OhPlan &P, int &code, std::string &err, Positions positions) {
    P.files.assign((size_t)nfiles, OhFile());
    P.jobs = 0;
    code = HB_EINVAL;
    for (uint64_t i = 0; i < nfiles; ++i) {
        OhFile &F = P.files[(size_t)i];
        memset(&F, 0, sizeof F);
        const std::string who = "file " + std::to_string(i) + ": ";
        if (d[i].num > 0xffffffffull || P.jobs + d[i].num > (1ull << 31)) {
            code = HB_EUNSUPPORTED;
            err = "more than 2^31 OneHash jobs in one call";
            return false;
        }
        if (!d[i].s0 || (!d[i].secret && d[i].secret_len) || (!d[i].data && d[i].len)) {
            err = who + "NULL buffer";
            return false;
        }
        if (!positions(i, who, code, err)) return false;
        F.len = F.file_size = d[i].len;
        F.job0 = P.jobs;
        F.n = (u32)d[i].num;
        oh_words(d[i].s0, F.s0);
        if (!hb_oh_secret(d[i].secret, d[i].secret_len, F.secret)) F.flags |= HB_OH_HOST_CHAIN;
        P.jobs += d[i].num;
    }
    if (P.jobs && (!seeds_out || !responses_out)) {
        err = "NULL buffer";
        return false;
    }
    code = 0;
    return true;
}

// hb_onehash_generate_many: the caller's blocks, each inside its file.
inline bool oh_plan_generate(const hb_onehash_gen_desc *d, uint64_t nfiles, const uint8_t *seeds_out,
                             const uint8_t *responses_out, OhPlan &P, int &code, std::string &err) {
    return oh_plan_files(d, nfiles, seeds_out, responses_out, P, code, err,
                         [d](uint64_t i, const std::string &who, int &, std::string &e) {
                             if (!d[i].blocks && d[i].num) {
                                 e = who + "NULL buffer";
                                 return false;
                             }
                             for (uint64_t k = 0; k < d[i].num; ++k)
                                 if (!oh_block_ok(d[i].blocks[k], d[i].len)) {
                                     e = who + "block " + std::to_string(d[i].blocks[k]) + " outside the file";
                                     return false;
                                 }
                             return true;
                         });
}

// The draws of a batch: the kernel's table and the files' keys, end to end.
struct OhDrawPlan {
    std::vector<OhDraw> draws;
    std::vector<u32> keys;
    uint64_t jobs = 0;
    bool states = false;   // a file asks for its final state
};

// One file's draw (len, key, num, blocks_out) as both entry points check it.
inline bool oh_draw_ok(uint64_t len, const uint32_t *key, uint64_t key_words, uint64_t num,
                       const uint64_t *blocks_out, const std::string &who, int &code, std::string &err) {
    if (key_words > HB_ONEHASH_MAX_KEY_WORDS) {
        code = HB_EUNSUPPORTED;
        err = who + "a key of more than " + std::to_string(HB_ONEHASH_MAX_KEY_WORDS) + " words";
        return false;
    }
    code = HB_EINVAL;
    if (len == 0 && num) {
        err = who + "no position in an empty range";
        return false;
    }
    if (key_words == 0) {
        err = who + "an empty key";
        return false;
    }
    if (!key || (!blocks_out && num)) {
        err = who + "NULL buffer";
        return false;
    }
    return true;
}

inline void oh_draw_add(OhDrawPlan &D, uint64_t len, const uint32_t *key, uint64_t key_words, uint64_t num,
                        const uint32_t *state_out) {
    OhDraw W;
    W.len = len;
    W.key0 = D.keys.size();
    W.key_words = key_words;
    W.job0 = D.jobs;
    W.num = num;
    D.draws.push_back(W);
    D.keys.insert(D.keys.end(), key, key + key_words);
    D.jobs += num;
    D.states |= state_out != nullptr;
}

// hb_onehash_pick_blocks_many: check every descriptor, then fill the table.
inline bool oh_plan_draw(const hb_onehash_draw_desc *d, uint64_t nfiles, OhDrawPlan &D, int &code,
                         std::string &err) {
    D = OhDrawPlan();
    uint64_t jobs = 0;
    if (nfiles >> 31) {
        code = HB_EUNSUPPORTED;
        err = "more than 2^31 OneHash jobs in one call";
        return false;
    }
    for (uint64_t i = 0; i < nfiles; ++i) {
        if (d[i].num > (1ull << 31) || jobs + d[i].num > (1ull << 31)) {
            code = HB_EUNSUPPORTED;
            err = "more than 2^31 OneHash jobs in one call";
            return false;
        }
        jobs += d[i].num;
        if (!oh_draw_ok(d[i].len, d[i].key, d[i].key_words, d[i].num, d[i].blocks_out,
                        "file " + std::to_string(i) + ": ", code, err))
            return false;
    }
    for (uint64_t i = 0; i < nfiles; ++i)
        oh_draw_add(D, d[i].len, d[i].key, d[i].key_words, d[i].num, d[i].state_out);
    code = 0;
    return true;
}

// hb_onehash_generate_drawn_many: hb_onehash_generate_many's checks with the
// draw's in the place of the blocks', and both tables.
inline bool oh_plan_generate_drawn(const hb_onehash_drawn_desc *d, uint64_t nfiles, const uint8_t *seeds_out,
                                   const uint8_t *responses_out, OhPlan &P, OhDrawPlan &D, int &code,
                                   std::string &err) {
    D = OhDrawPlan();
    if (nfiles >> 31) {
        code = HB_EUNSUPPORTED;
        err = "more than 2^31 OneHash jobs in one call";
        return false;
    }
    if (!oh_plan_files(d, nfiles, seeds_out, responses_out, P, code, err,
                       [d](uint64_t i, const std::string &who, int &c, std::string &e) {
                           return oh_draw_ok(d[i].len, d[i].key, d[i].key_words, d[i].num, d[i].blocks_out, who, c, e);
                       }))
        return false;
    for (uint64_t i = 0; i < nfiles; ++i)
        oh_draw_add(D, d[i].len, d[i].key, d[i].key_words, d[i].num, d[i].state_out);
    code = 0;
    return true;
}

// hb_onehash_meet_many: check every file and job, and order the jobs file by
// file (order[j]: the caller's index of sorted job j).
inline bool oh_plan_meet(const hb_onehash_file *files, uint64_t nfiles, const hb_onehash_job *jobs,
                         uint64_t njobs, const uint8_t *responses_out, OhPlan &P, std::vector<size_t> &order,
                         int &code, std::string &err) {
    P.files.assign((size_t)nfiles, OhFile());
    P.jobs = njobs;
    order.assign((size_t)njobs, 0);
    code = HB_EINVAL;
    if (njobs > (1ull << 31)) {
        code = HB_EUNSUPPORTED;
        err = "more than 2^31 OneHash jobs in one call";
        return false;
    }
    if (!files || !jobs || !responses_out) {
        err = "NULL buffer";
        return false;
    }
    for (uint64_t i = 0; i < nfiles; ++i) {
        OhFile &F = P.files[(size_t)i];
        memset(&F, 0, sizeof F);
        if (!files[i].data && files[i].len) {
            err = "file " + std::to_string(i) + ": NULL buffer";
            return false;
        }
        F.len = F.file_size = files[i].len;
    }
    for (uint64_t j = 0; j < njobs; ++j) {
        const std::string who = "job " + std::to_string(j) + ": ";
        if (jobs[j].file >= nfiles) {
            err = who + "no file " + std::to_string(jobs[j].file);
            return false;
        }
        if (jobs[j].seed_len > HB_ONEHASH_MAX_SEED) {
            err = who + "seed longer than 64 bytes";
            return false;
        }
        if (!oh_block_ok(jobs[j].block, files[jobs[j].file].len)) {
            err = who + "block " + std::to_string(jobs[j].block) + " outside the file";
            return false;
        }
        ++P.files[(size_t)jobs[j].file].n;
    }
    uint64_t at = 0;
    std::vector<uint64_t> next((size_t)nfiles);
    for (uint64_t i = 0; i < nfiles; ++i) {
        P.files[(size_t)i].job0 = next[(size_t)i] = at;
        at += P.files[(size_t)i].n;
    }
    for (uint64_t j = 0; j < njobs; ++j) order[(size_t)next[(size_t)jobs[j].file]++] = (size_t)j;
    code = 0;
    return true;
}

// SHA-256(s || secret) for a secret of any length: the host chain's link.
inline void oh_link_any(const uint8_t *secret, uint64_t secret_len, std::vector<uint8_t> &msg, u32 s[8]) {
    msg.resize(32 + (size_t)secret_len);
    oh_bytes(s, msg.data());
    if (secret_len) memcpy(msg.data() + 32, secret, (size_t)secret_len);
    hb_mk_init(s);
    hb_mk_sha256_tail(s, 0, msg.data(), msg.size());
}

// The n seeds of a file into seeds (n x 32 bytes): what
// hb_onehash_chain_kernel writes, on the host, for a secret of any length.
inline void oh_host_chain(const OhFile &F, const uint8_t *secret, uint64_t secret_len, uint8_t *seeds) {
    u32 s[8], nx[8];
    for (int t = 0; t < 8; ++t) s[t] = F.s0[t];
    std::vector<uint8_t> msg;
    for (u32 k = 0; k < F.n; ++k) {
        oh_bytes(s, seeds + (size_t)k * 32);
        if (k + 1 == F.n) break;
        if (F.flags & HB_OH_HOST_CHAIN) {
            oh_link_any(secret, secret_len, msg, s);
        } else {
            hb_oh_link(F.secret, s, nx);
            for (int t = 0; t < 8; ++t) s[t] = nx[t];
        }
    }
}

// The segments of one job of a gathered file into its slot of chunk bytes:
// the first at the slot's start, the second right after it.  False when a
// segment lies outside the file's len bytes.
inline bool oh_gather_job(const uint8_t *data, uint64_t len, uint64_t block, uint8_t *slot) {
    const HbOhPlan P = hb_oh_plan(len, block);
    if (!hb_oh_plan_inside(P, len)) return false;
    if (P.len0) memcpy(slot, data + P.off0, (size_t)P.len0);
    if (P.len1) memcpy(slot + P.len0, data + P.off1, (size_t)P.len1);
    return true;
}

}  // namespace hbhost
