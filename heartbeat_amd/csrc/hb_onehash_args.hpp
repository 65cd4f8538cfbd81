// hb_onehash_args.hpp -- the OneHash scheme's kernel arguments and per-file
// device table (hb_kern_onehash.hip, hb_runtime.cpp, hb_onehash_host.hpp).
#pragma once
#include "hb_onehash.hpp"
#include "hb_onehash_draw.hpp"

// OhFile::flags
#define HB_OH_GATHER 1u       // a host file too large to upload: data holds its jobs' segments
                              // only, job k of the file at k * chunk, the second right after the first
#define HB_OH_HOST_CHAIN 2u   // the chain kernel leaves this file's seeds alone (a secret above 87 bytes)

// One file of hb_onehash_generate_many or hb_onehash_meet_many: the state a
// lane needs, indexed by file number.  Jobs are numbered file by file.
struct OhFile {
    const unsigned char *data;   // the bytes the segments are read from (device)
    u64 len;                     // readable bytes at data
    u64 file_size;               // the size the plan rule is run for
    u64 job0;                    // the file's first flat job index
    u32 n, flags;                // jobs of the file; HB_OH_*
    u32 s0[8];                   // chain: the first seed, SHA-256(root seed)
    HbOhSecret secret;           // chain: the prepared secret
};

// hb_onehash_chain_kernel: a lane per file writes its n seeds.
struct OhChainArgs {
    const OhFile *files;
    u64 nfiles;
    u32 *seeds;                  // [jobs] x 32 bytes
};

// hb_onehash_resp_kernel: a lane per job.  Blocks, seeds and seed lengths are
// strided arrays, so that one kernel reads the generate side's packed blocks
// and chain seeds and the meet side's job records.
struct OhRespArgs {
    const OhFile *files;
    u64 nfiles, njobs;
    const unsigned char *blocks;      // job j's block: a u64 at blocks + j * block_stride
    u64 block_stride;
    const unsigned char *seeds;       // job j's seed bytes at seeds + j * seed_stride
    u64 seed_stride;
    const unsigned char *seed_lens;   // job j's seed length: a u64 at seed_lens + j * len_stride; NULL: 32
    u64 len_stride;
    u32 *resp;                        // [jobs] x 32 bytes
    unsigned int *flags;              // bit 2: a segment outside its buffer, or a seed too long
};

// One file of hb_onehash_draw_kernel: num positions in [0, len) from the
// generator seeded with keys[key0 : key0 + key_words].
struct OhDraw {
    u64 len;
    u64 key0, key_words;         // the file's key in the batch's key array
    u64 job0, num;               // its positions at blocks[job0 : job0 + num]
};

// hb_onehash_draw_kernel: a wave per file.
struct OhDrawArgs {
    const OhDraw *draws;
    u64 nfiles;
    const u32 *keys;
    u64 *blocks;                 // [jobs]
    u32 *states;                 // [nfiles] x HB_MT_STATE_WORDS, or NULL
};
