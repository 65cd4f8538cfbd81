// hb_cpv_args.hpp -- argument blocks and table entries of the batched cxx
// prove and verify (hb_cpv.hpp), shared with the host runtime.  Apart from
// hb_args.hpp so that these units rebuild alone.  The wave-job table entry,
// the kinds and HB_CB_JOB come from the planner's header.
#pragma once
#include "hb_args.hpp"
#include "hb_cbatch_plan.hpp"

// hb_cxx_prove_many / hb_cxx_verify_rhs_many: one entry per item of a group.
struct CpvItem {
    u64 obase;                    // the item's first challenge index in the group's idx, v and F buffers
    u64 range;                    // the index prf's limit: ntags (prove), state_chunks (verify)
    u32 chunks;                   // effective challenge length (range when check_all)
    u32 flags;                    // HB_CPV_ALL
};
// check_all (cxx/shacham_waters_private.cxx:754-755, 822-827): every block in
// order, idx_i = i, no index prf
#define HB_CPV_ALL 1u

// Schedules of an item in CpvPrfArgs::prf, at stride * item + slot (prove:
// stride 1, the v schedule only; verify: stride 3).
#define HB_CPV_PV 0u              // cxx prf(chal_key, v_max)
#define HB_CPV_PF 1u              // cxx prf(f_key, p)
#define HB_CPV_PA 2u              // cxx prf(alpha_key, p)

template <int NL>
struct CpvPrfArgs {
    const PrfParams<2> *pidx;     // [item]: cxx prf(chal_key, range), byte-granular tries
    const PrfParams<NL> *prf;     // [stride item + slot]
    const CpvItem *items;
    const HbCbJob *jobs;
    u64 njobs;
    u64 *idx;                     // HB_CB_IDX: idx_i of item f at obase + i (0 when out of range)
    u32 *status;                  // [item]: bit 0 = an index the forced accept left >= range (prove)
    u32 *vv;                      // HB_CB_V: v_i at (obase + i) * NL, little-endian limbs, raw
    u32 *fv;                      // HB_CB_IDXF: F(idx_i), same place
    u32 *av;                      // HB_CB_ALPHA: alpha_j of item f at (f * S + j) * NL, raw
    u32 S, stride;
    const u32 *t0;
    unsigned long long *queue;    // slot k = kind (queue + k HB_QSLOT): [1] tries; slot 0 [0]: next wave-job
};

// One file of a group of hb_cxx_prove_many.
struct CpvFile {
    const unsigned char *data;    // the whole file (device), any alignment
    u64 len;
    const unsigned char *tags;    // ntags * tw big-endian bytes (device), any alignment
    u64 ntags;
    u64 obase;
    u32 chunks;
    u32 flags;                    // HB_CPV_ALL, HB_CPV_LOAD16
};
// full-width sectors and tags (ss == tw == 4 NL) with the file, the tag array
// and C all 16-byte aligned: whole sectors and tags are 16-byte loads.  An
// offset taken mod 2^32 keeps that alignment.
#define HB_CPV_LOAD16 2u

template <int NL>
struct CpvSumArgs {
    ModP<NL> mod;
    const CpvFile *files;         // nfiles * (S + 1) workgroups: (file, column)
    const u64 *idx;               // not read for a check_all file
    const u32 *vm;                // v_i R mod p (hb_mont_kernel over the PRF launch's vv), same place
    u32 *res;                     // column j of file f at (f * (S + 1) + j) * NL; j = S: sigma
    u64 C;
    u32 ss, S, tw;
};
