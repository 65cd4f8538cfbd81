// hb_vbatch_args.hpp -- argument blocks and table entries of the batched
// verify's kernels (hb_vbatch.hpp), shared with the host runtime.  Apart from
// hb_args.hpp so that the batched verify's units rebuild alone.
#pragma once
#include "hb_args.hpp"

// hb_verify_rhs_many: many small proofs, each under its own f_key, alpha_key
// and challenge key, in one PRF launch and one sum launch per group.  As in
// the batched encode the per-proof state lives in device tables indexed by a
// wave-uniform proof number; only what the whole batch shares (the prime, S)
// is in the kernel arguments.  Here the PRF ranges differ per proof as well
// (state_chunks, v_max), so R, nb and topmask are per table entry.
struct VbProof {
    u64 obase;                    // the proof's first challenge index in the group's v and F buffers
    u32 chunks;
    u32 pad_;
};

// One quad-engine wave's work: up to 16 evaluations [first, first + count) of
// one proof.
#define HB_VB_IDXF 0u             // idx_i = KeyedPRF(chal_key, state_chunks)(i), then F(idx_i)
#define HB_VB_V 1u                // v_i = KeyedPRF(chal_key, v_max)(i)
#define HB_VB_ALPHA 2u            // alpha_j = KeyedPRF(alpha_key, p)(j)
struct VbWaveJob {
    u32 proof, kind, first, count;
};

template <int NL>
struct VbPrfArgs {
    const PrfParams<2> *pidx;     // [proof]: KeyedPRF(chal_key, state_chunks)
    const PrfParams<NL> *prf;     // [3 proof + kind]: F (f_key, p), v (chal_key, v_max), alpha (alpha_key, p)
    const VbProof *proofs;
    const VbWaveJob *jobs;
    u64 njobs;
    u32 *fv;                      // F(idx_i) of proof f at (obase + i) * NL, little-endian limbs
    u32 *vv;                      // v_i, same place
    u32 *av;                      // alpha_j of proof f at (f * S + j) * NL
    u32 S;
    const u32 *t0;
    unsigned long long *queue;    // slot k = kind (queue + k HB_QSLOT): [1] tries, [2] abandoned jobs
                                  // (kind 0: of the index and the F engine); slot 0 [0]: next wave-job
};

template <int NL>
struct VbSumArgs {
    ModP<NL> mod;
    u32 r2[NL];                   // R^2 mod p
    const VbProof *proofs;        // one workgroup per entry
    const u32 *fv, *vv, *av;
    const u32 *mu;                // mu_j of proof f at (f * S + j) * NL, little-endian limbs
    u32 *res;                     // rhs of proof f at f * NL
    u32 S;
};
