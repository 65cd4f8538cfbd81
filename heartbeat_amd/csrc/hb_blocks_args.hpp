// hb_blocks_args.hpp -- kernel arguments of the listed-block encode
// (hb_encode_blocks_many; hb_kern_blocks.hip, hb_runtime.cpp).
//
// A file's listed blocks are packed back to back, so to the MAC they are a
// small file of their own: the batched encode's BatchFile, BatchWaveJob,
// BatchMacWg and BatchMacArgs (hb_args.hpp) serve unchanged.  What differs is
// the PRF input: F is evaluated at the block's index in the owner's file,
// which the packed position does not tell.  BatchPrfArgs has no room for the
// index table and hb_batch_prf_kernel must keep its arguments, hence a struct
// of its own.
#pragma once
#include "hb_args.hpp"

template <int NL>
struct BlocksPrfArgs {
    const PrfParams<NL> *prf;     // [2 file + kind]: KeyedPRF(f_key, p), KeyedPRF(alpha_key, p)
    const BatchFile *files;       // fbase: the file's first listed block in idx and in fv
    const BatchWaveJob *jobs;     // kind 0: F of listed blocks [first, first + count); kind 1: alpha_j
    u64 njobs;
    ModP<NL> mod;
    u32 r2[NL];                   // R^2 mod p
    const u64 *idx;               // idx[fbase + k]: index of the file's k-th listed block, any u64
    u32 *fv;                      // F(idx[fbase + k]) at (fbase + k) * NL, little-endian limbs
    u32 *amont;                   // alpha_j R mod p of file f at (f * S + j) * NL
    u32 S;
    const u32 *t0;
    unsigned long long *queue;    // as BatchPrfArgs: slot 0 the wave-job counter and F's tries,
                                  // slot 1 (queue + HB_QSLOT) alpha's
};
