// hb_cmixed_args.hpp -- argument blocks of the cxx mixed-owner batches'
// kernels (hb_cmixed.hpp: hb_cxx_prove_mixed, hb_cxx_verify_rhs_mixed), shared
// with the host runtime.  Apart from hb_cpv_args.hpp and hb_mixed_args.hpp so
// that the cxx mixed units rebuild alone and neither of those units' inputs
// change.
#pragma once
#include "hb_cpv_args.hpp"
#include "hb_mixed_args.hpp"

// A proof of hb_cxx_prove_mixed has two table entries.  The PRF launch
// (hb_cpv_prf_kernel, unchanged) reads its CpvItem, flags HB_CPV_ALL (1).  The
// conversion pass (hb_mixed_mont_kernel, unchanged: it reads obase and chunks
// only) and the sum launch read its PbProof, whose flags are HB_PB_LOAD16 (1)
// and, for check_all, HB_CMX_ALL: a bit of its own, because HB_CPV_ALL and
// HB_PB_LOAD16 are both 1 and this table is the one both passes share.
// PbProof::chunks is the EFFECTIVE challenge length (ntags when check_all).
#define HB_CMX_ALL 2u

// The sum launch: MxSumArgs (hb_mixed_args.hpp) as it is -- the records, the
// PbProof table, one MxWg (proof, column) per workgroup, idx (not read for a
// check_all proof), v R mod p_f, and the results at (col0_f + j) * NL.
template <int NL>
using CmSumArgs = MxSumArgs<NL>;

// The verify's PRF launch takes CpvPrfArgs as it is (S is not read): alpha_j
// of proof f lands at (slot0_f + j) * NL, and slot0_f travels in the table the
// kernel reads anyway, above the flag bit: CpvItem::flags = HB_CPV_ALL |
// slot0_f << HB_CMX_SLOT_SHIFT (slot0 < 2^31: each slot costs NL 4 >= 32 bytes
// of a group's HB_BATCH_BYTES).  The kernel reads it through the table at the
// one place it is used (hb_cmixed.hpp CmAlphaOwn), so the launch needs no
// pointer to the records and keeps no more scalar registers live than
// hb_cpv_prf_kernel: scratch use is the sibling's in every instantiation.
#define HB_CMX_SLOT_SHIFT 1u
