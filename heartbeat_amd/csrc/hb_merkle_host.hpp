// hb_merkle_host.hpp -- host side of hb_merkle_encode_many and
// hb_merkle_leaves_many (pure C++, no HIP calls): the descriptor checks, the
// per-file table the kernels index, the host seed chain, and which host files
// are uploaded whole and which are gathered.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/hbswizzle.h"
#include "hb_merkle_args.hpp"

namespace hbhost {

// Files from which the device chain beats the host's.  One lane walks a
// file's chain whatever the batch, so the device costs a constant (a 256-link
// chain: 1.3 ms of kernel, calls of about 1.5 ms + 0.009 ms per file) where
// the host pays per file (0.08 ms each on one thread, calls of about 0.2 ms +
// 0.08 ms per file): the host wins at 16 files (1.5 against 1.65 ms), the
// device at 64 (2.1 against 5.3 ms), and the two lines cross between 17 and
// 18 (profiles/many/merkle_rate.json, "chain").
const uint64_t MK_CHAIN_DEVICE_MIN_FILES = 18;

// A host file is uploaded whole up to this many bytes, the threshold the cxx
// prove's gather uses; above it only the chunks go to the device.
inline uint64_t mk_upload_max(uint64_t n, uint64_t chunk) {
    const uint64_t floor = 8ull << 20;
    if (chunk && n > (~0ull / 2) / chunk) return ~0ull;
    const uint64_t twice = 2 * n * chunk;
    return twice > floor ? twice : floor;
}

struct MkPlan {
    std::vector<MkFile> files;
    uint64_t jobs = 0;    // leaves of all files
    uint64_t nodes = 0;   // node entries of all files
};

// The range, clamp and PRF shape of one file (Merkle.py:497-503).  code / err
// as the C ABI reports them.
inline bool mk_fill_range(MkFile &F, uint64_t filesz, uint64_t chunksz, uint64_t len, int &code,
                          std::string &err) {
    if (filesz > len) {
        code = HB_EINVAL;
        err = "chunk past the end of the data";
        return false;
    }
    const uint64_t chunk = chunksz > filesz ? filesz : chunksz;
    const uint64_t range = filesz - chunk + 1;
    if (range == 0) {
        code = HB_EUNSUPPORTED;
        err = "Merkle chunk range of 2^64";
        return false;
    }
    F.chunk = chunk;
    F.R[0] = (u32)range;
    F.R[1] = (u32)(range >> 32);
    int bits = 0;
    for (uint64_t r = range; r; r >>= 1) ++bits;
    F.nb = (u32)(bits + 7) / 8;
    F.topmask = (1u << (bits - 8 * ((int)F.nb - 1))) - 1u;
    return true;
}

// Check every descriptor and fill the table (data pointers are the runtime's).
inline bool mk_plan_encode(const hb_merkle_encode_desc *d, uint64_t nfiles, MkPlan &P, int &code,
                           std::string &err) {
    P.files.assign((size_t)nfiles, MkFile());
    P.jobs = P.nodes = 0;
    for (uint64_t i = 0; i < nfiles; ++i) {
        MkFile &F = P.files[(size_t)i];
        memset(&F, 0, sizeof F);
        code = HB_EINVAL;
        if (d[i].n < 1 || d[i].n > HB_MERKLE_MAX_N) {
            err = "file " + std::to_string(i) + ": n must be in 1..65536 on the GPU path";
            return false;
        }
        if ((!d[i].key && d[i].key_len) || (!d[i].seed && d[i].seed_len) || !d[i].nodes_out ||
            (!d[i].data && d[i].filesz)) {
            err = "NULL buffer";
            return false;
        }
        if (!mk_fill_range(F, d[i].filesz, d[i].chunksz, d[i].len, code, err)) return false;
        F.n = (u32)d[i].n;
        F.order = hb_mk_order(d[i].n);
        F.seed_len = 32;
        F.job0 = P.jobs;
        F.node0 = P.nodes;
        P.jobs += d[i].n;
        P.nodes += 2ull << F.order;
        hb_mk_key(d[i].key, d[i].key_len, F.key);
        hb_mk_hmac(F.key, d[i].seed, d[i].seed_len, F.s1);
    }
    code = 0;
    return true;
}

// The n leaf seeds of a file into seeds (n x 32 bytes): what
// hb_merkle_chain_kernel writes, on the host.
inline void mk_host_chain(const MkFile &F, uint8_t *seeds) {
    u32 s[8], nx[8];
    for (int t = 0; t < 8; ++t) s[t] = F.s1[t];
    for (u32 k = 0; k < F.n; ++k) {
        for (int t = 0; t < 8; ++t)
            for (int b = 0; b < 4; ++b) seeds[(size_t)k * 32 + 4 * t + b] = (uint8_t)(s[t] >> (24 - 8 * b));
        if (k + 1 < F.n) {
            hb_mk_link(F.key, s, nx);
            for (int t = 0; t < 8; ++t) s[t] = nx[t];
        }
    }
}

}  // namespace hbhost
