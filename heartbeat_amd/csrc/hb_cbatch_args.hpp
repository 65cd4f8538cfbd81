// hb_cbatch_args.hpp -- argument block of the batched cxx PRF launch
// (hb_cbatch.hpp), shared with the host runtime.  Apart from hb_args.hpp so
// that the batched cxx units rebuild alone.  The wave-job table entry and
// HB_CB_JOB come from the planner's header.
#pragma once
#include "hb_args.hpp"
#include "hb_cbatch_plan.hpp"

// A file whose length is a multiple of C has a last block that reads no
// sector (block len / C starts at the end of the file).  The cxx encode leaves
// that tag as the PRF returned it, without `%= p`
// (cxx/shacham_waters_private.cxx:681-690), so the PRF launch stores it (any
// F block k with k C >= len) and the file's BatchFile::nblocks counts one block
// less: the MAC launch never sees it.
template <int NL>
struct CbPrfArgs {
    const PrfParams<NL> *prf;     // [2 item + kind]: cxx prf(f_key, p), cxx prf(alpha_key, p)
    const BatchFile *files;       // nblocks: the blocks the MAC launch tags (see above)
    const HbCbJob *jobs;
    u64 njobs;
    u32 *fv;                      // F(k) of item f at (fbase + k) * NL, little-endian limbs
    u32 *araw;                    // alpha_j of item f at (f * S + j) * NL, raw (hb_mont_kernel follows)
    u64 C;
    u32 S, tw;
    const u32 *t0;
    unsigned long long *queue;    // slot k = kind (queue + k HB_QSLOT): [1] tries; slot 0 [0]: next wave-job
};
