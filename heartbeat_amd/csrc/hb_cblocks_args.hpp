// hb_cblocks_args.hpp -- kernel arguments of the cxx listed-block encode
// (hb_cxx_encode_blocks_many; hb_kern_cblocks.hip, hb_runtime.cpp).
//
// A file's listed blocks are packed back to back, so to the MAC they are a
// small file of their own: the batched encodes' BatchFile, BatchMacWg and
// BatchMacArgs (hb_args.hpp) and the cxx batch's wave-job (HbCbJob,
// hb_cbatch_plan.hpp) serve unchanged.  What differs is the PRF input: F is
// evaluated at the block's index in the owner's file, which the packed
// position does not tell.  CbPrfArgs has no room for the index table and
// hb_cbatch_prf_kernel must keep its arguments, hence a struct of its own.
//
// The block that reads no sector keeps F unreduced as in the cxx batch
// (hb_cbatch_args.hpp): it is a matter of the packed position -- at most the
// last listed block of a list, so of the list's last segment -- and that
// segment's BatchFile::nblocks counts one block less than its F evaluations.
#pragma once
#include "hb_args.hpp"
#include "hb_cbatch_plan.hpp"

template <int NL>
struct CblkPrfArgs {
    const PrfParams<NL> *prf;     // [2 item + kind]: cxx prf(f_key, p), cxx prf(alpha_key, p)
    const BatchFile *files;       // fbase: the item's first listed block in idx and in fv; nblocks: the MAC's
    const HbCbJob *jobs;          // HB_CB_F: F of listed blocks [first, first + count); HB_CB_ALPHA: alpha_j
    u64 njobs;
    const u32 *idx;               // idx[fbase + k]: index of the item's k-th listed block (the cxx prf's unsigned int)
    u32 *fv;                      // F(idx[fbase + k]) at (fbase + k) * NL, little-endian limbs
    u32 *araw;                    // alpha_j of item f at (f * S + j) * NL, raw (hb_mont_kernel follows)
    u64 C;
    u32 S, tw;
    const u32 *t0;
    unsigned long long *queue;    // as CbPrfArgs: slot k = kind, [1] tries; slot 0 [0]: next wave-job
};
