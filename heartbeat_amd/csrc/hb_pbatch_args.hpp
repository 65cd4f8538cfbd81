// hb_pbatch_args.hpp -- argument blocks and table entries of the batched
// prove's kernels (hb_pbatch.hpp), shared with the host runtime.  Apart from
// hb_args.hpp so that the batched prove's units rebuild alone.
#pragma once
#include "hb_args.hpp"

// hb_prove_many: many small proofs, each under its own challenge key, file and
// tag array, in one PRF launch and one sum launch per group.  As in the
// batched verify the per-proof state lives in device tables indexed by a
// wave-uniform proof number; only what the whole batch shares (the prime, S,
// the sector geometry) is in the kernel arguments.
struct PbProof {
    u64 obase;                    // the proof's first challenge index in the group's idx and v buffers
    const unsigned char *data;    // the whole file (device), any alignment
    u64 len;
    const unsigned char *tags;    // ntags * tw big-endian bytes (device), any alignment
    u64 ntags;
    u32 chunks;
    u32 flags;                    // HB_PB_LOAD16
};
// full-width sectors and tags (ss == tw == 4 NL) with the file, the tag array
// and C all 16-byte aligned: whole sectors and tags are 16-byte loads
// (hb_load_full16) instead of byte loads
#define HB_PB_LOAD16 1u

// One quad-engine wave's work: up to 16 evaluations [first, first + count) of
// one proof.  The kind is also the wave-job's queue slot (tries, abandoned jobs).
#define HB_PB_IDX 0u              // idx_i = KeyedPRF(chal_key, ntags)(i)
#define HB_PB_V 1u                // v_i = KeyedPRF(chal_key, v_max)(i)
struct PbWaveJob {
    u32 proof, kind, first, count;
};

template <int NL>
struct PbPrfArgs {
    const PrfParams<2> *pidx;     // [proof]: KeyedPRF(chal_key, ntags)
    const PrfParams<NL> *pv;      // [proof]: KeyedPRF(chal_key, v_max)
    const PbProof *proofs;
    const PbWaveJob *jobs;
    u64 njobs;
    u64 *idx;                     // idx_i of proof f at obase + i
    u32 *vv;                      // v_i of proof f at (obase + i) * NL, little-endian limbs, raw
    const u32 *t0;
    unsigned long long *queue;    // slot k = kind (queue + k HB_QSLOT): [1] tries, [2] abandoned jobs;
                                  // slot 0 [0]: next wave-job
};

template <int NL>
struct PbSumArgs {
    ModP<NL> mod;
    const PbProof *proofs;        // gridDim.y entries; gridDim.x = S + 1 columns
    const u64 *idx;
    const u32 *vm;                // v_i R mod p (hb_mont_kernel over the PRF launch's vv), same place
    u32 *res;                     // column j of proof f at (f * (S + 1) + j) * NL; j = S: sigma
    u64 C;
    u32 ss, S, tw;
};
