// hb_merkle_args.hpp -- the Merkle scheme's kernel arguments and per-file
// device table (hb_kern_merkle.hip, hb_runtime.cpp, hb_merkle_host.hpp).
#pragma once
#include "hb_merkle.hpp"

// MkFile::flags
#define HB_MK_GATHER 1u   // a host file too large to upload: pass 0 writes its positions
                          // only; pass 1 hashes the gathered chunks, leaf k at k * chunk

// One file of hb_merkle_encode_many, or one proof of hb_merkle_leaves_many
// (a "file" of one leaf): the state a lane needs, indexed by file number.
struct MkFile {
    const unsigned char *data;   // the bytes the chunks are read from (device); NULL: positions only
    u64 len;                     // readable bytes at data
    u64 chunk;                   // min(chunksz, filesz) (Merkle.py:500-501)
    u64 job0;                    // the file's first flat job (leaf) index
    u64 node0;                   // its first node in the node buffer, in 32-byte entries
    u32 n, order;                // leaves, tree order
    u32 R[2];                    // KeyedPRF range filesz - chunk + 1, two little-endian limbs
    u32 nb, topmask;             // keystream bytes per try, mask of the top byte (util.py:66-81)
    u32 seed_len, flags;         // bytes of a seed (16, 24 or 32); HB_MK_*
    HbMkKey key;                 // chain: the key's HMAC midstates
    u32 s1[8];                   // chain: the first link, HMAC(key, caller's seed)
};

// hb_merkle_chain_kernel: a lane per file writes its n leaf seeds.
struct MkChainArgs {
    const MkFile *files;
    u64 nfiles;
    u32 *seeds;                  // [jobs] x 32 bytes
};

// hb_merkle_leaves_kernel<NR>: a lane per job in [job_lo, job_hi), all of whose
// seeds have the length that NR stands for.
struct MkLeavesArgs {
    const MkFile *files;
    u64 nfiles;
    u64 job_lo, job_hi;
    u32 pass;                    // 0: every file (HB_MK_GATHER ones: positions only); 1: HB_MK_GATHER ones only
    const u32 *seeds;            // [jobs] x 32 bytes, a seed at the start of its slot
    u64 *offsets;                // [jobs] chunk positions: written by pass 0, read by pass 1
    u32 *blobs;                  // [jobs] x 32 bytes: HMAC-SHA256(seed, chunk), the leaf blobs
    u32 *nodes;                  // node buffer (NULL: no leaf hashes, the prove side)
    u32 dig0[8];                 // SHA-256("0"): eval(0) hashes str(0) (util.py:91)
    unsigned int *flags;         // bit 1: a PRF did not terminate; bit 2: a chunk outside its buffer
    const u32 *t0;
};

// hb_merkle_tree_kernel: a workgroup per file, level by level up to the root.
struct MkTreeArgs {
    const MkFile *files;
    u32 *nodes;
};
