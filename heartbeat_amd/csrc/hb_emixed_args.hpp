// hb_emixed_args.hpp -- argument blocks of the mixed-owner encodes' kernels
// (hb_emixed.hpp: hb_encode_mixed, hb_cxx_encode_mixed), shared with the host
// runtime.  Apart from hb_args.hpp so that the mixed encode's units rebuild
// alone.
#pragma once
#include "hb_cbatch_args.hpp"
#include "hb_mixed_args.hpp"

// A file of a mixed encode names its own prime and sector count.  What
// hb_encode_many keeps in the kernel arguments (the modulus, C, ss, S, tw) is
// the file's MxRec, the record of the mixed prove and verify, in a device table
// indexed by the same wave-uniform file number as BatchFile; slot0 is the
// file's first alpha slot (sum of S_g over the files before it), which the
// one-prime calls compute as file * S.  col0 is not used.  The file table, the
// key schedules ([2 file + kind], each with its own R = p_f, nb and topmask),
// the wave-jobs and the MAC workgroup entries are hb_encode_many's and
// hb_cxx_encode_many's.

// PySwizzle side: hb_batch_prf_kernel's arguments without the modulus.  alpha
// is stored as the PRF returned it; hb_mixed_mont_kernel converts the group's
// slots under each file's modulus afterwards (hb_emixed.hpp: why).
template <int NL>
struct EmPrfArgs {
    const PrfParams<NL> *prf;     // [2 file + kind]: KeyedPRF(f_key, p_f), KeyedPRF(alpha_key, p_f)
    const BatchFile *files;
    const BatchWaveJob *jobs;
    u64 njobs;
    const MxRec<NL> *recs;
    u32 *fv;                      // F(k) of file f at (fbase_f + k) * NL, little-endian limbs
    u32 *araw;                    // alpha_j of file f at (slot0_f + j) * NL, raw
    const u32 *t0;
    unsigned long long *queue;    // as BatchPrfArgs::queue
};

// cxx side: CbPrfArgs with C, tw and the alpha slot from the file's record
template <int NL>
struct CemPrfArgs {
    const PrfParams<NL> *prf;     // [2 item + kind]: cxx prf(f_key, p_f), cxx prf(alpha_key, p_f)
    const BatchFile *files;       // nblocks: the blocks the MAC launch tags (hb_cbatch_args.hpp)
    const HbCbJob *jobs;
    u64 njobs;
    const MxRec<NL> *recs;
    u32 *fv;
    u32 *araw;                    // alpha_j of item f at (slot0_f + j) * NL, raw
    const u32 *t0;
    unsigned long long *queue;    // as CbPrfArgs::queue
};

// The MAC launches of both (one per shape, hb_emixed.hpp): one workgroup per
// entry of wgs; the entry's blocks are [first, first + hb_em_bpw(T, S_file)).
template <int NL>
struct EmMacArgs {
    const MxRec<NL> *recs;
    const BatchFile *files;
    const BatchMacWg *wgs;
    const u32 *fv;
    const u32 *amont;             // alpha_j R mod p_f of file f at (slot0_f + j) * NL
};
