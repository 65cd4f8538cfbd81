// hb_mixed_args.hpp -- argument blocks and table entries of the mixed-owner
// batches' kernels (hb_mixed.hpp: hb_prove_mixed, hb_verify_rhs_mixed), shared
// with the host runtime.  Apart from hb_args.hpp so that the mixed units
// rebuild alone.
#pragma once
#include "hb_pbatch_args.hpp"
#include "hb_vbatch_args.hpp"

// A proof of a mixed batch names its own prime and sector count.  What the
// one-prime batches keep in the kernel arguments (the modulus, R^2 mod p, C,
// ss, S, tw) is a record per proof in a device table, indexed by the same
// wave-uniform proof number as PbProof / VbProof; so are the places that used
// to follow from a common S: the proof's first result column (prove) and its
// first alpha / mu slot (verify).  The kernels read a record's modulus through
// a wave-uniform pointer into the table (hb_table_ref), never by value.
template <int NL>
struct MxRec {
    ModP<NL> mod;
    u32 r2[NL];                   // R^2 mod p
    u64 C;                        // S * ss
    u32 ss, S, tw;
    u32 col0;                     // prove: the proof's first result column (sum of S_g + 1 over the proofs before it)
    u32 slot0;                    // verify: the proof's first alpha and mu slot (sum of S_g)
    u32 pad_;
};

// One workgroup's work.  Sum launch of the prove: column `a` of the proof
// (a == S: sigma).  Conversion pass: terms [a, a + 256) of the proof, so a
// workgroup never holds terms of two proofs.
struct MxWg {
    u32 proof, a;
};
#define HB_MX_MONT_WG 256u

// v -> v R mod p over a group's v buffer, in place, under each proof's modulus
template <int NL>
struct MxMontArgs {
    const MxRec<NL> *recs;
    const PbProof *proofs;
    const MxWg *wgs;              // one entry per workgroup
    u32 *vv;
};

template <int NL>
struct MxSumArgs {
    const MxRec<NL> *recs;
    const PbProof *proofs;
    const MxWg *wgs;              // one entry per workgroup: sum of S_f + 1 over the group
    const u64 *idx;
    const u32 *vm;                // v_i R mod p_f
    u32 *res;                     // column j of proof f at (col0_f + j) * NL; j = S_f: sigma
};

// hb_vbatch_prf_kernel's arguments (S is not read) and the records: alpha_j of
// proof f lands at (slot0_f + j) * NL
template <int NL>
struct VmPrfArgs {
    VbPrfArgs<NL> b;
    const MxRec<NL> *recs;
};

template <int NL>
struct VmSumArgs {
    const MxRec<NL> *recs;
    const VbProof *proofs;        // one workgroup per entry
    const u32 *fv, *vv, *av;
    const u32 *mu;                // mu_j of proof f at (slot0_f + j) * NL, little-endian limbs
    u32 *res;                     // rhs of proof f at f * NL
};
