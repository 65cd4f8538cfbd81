// hb_cmixed.hpp -- kernels of the cxx mixed-owner batches (hb_cxx_prove_mixed,
// hb_cxx_verify_rhs_mixed; instantiated by hb_kern_cmixed.hip and
// hb_kern_cmixed64.hip): the batched cxx prove and verify of hb_cpv.hpp for
// proofs that each name their own prime and sector count.  Replaces a storage
// node's loop over cxx/shacham_waters_private.cxx:731-789 for the challenges
// of many owners (every Swizzle draws its own prime, :596-624) and an
// auditor's loop over :791-842, both with the cxx prf (cxx/prf.hxx:125-176).
//
// Launches of a group and where their kernels live:
//   prove   PRF         hb_cpv_prf_kernel (hb_cpv.hpp) as it is: its V and IDX
//                       kinds take the limit, nb and topmask from the item's
//                       own schedules and write at obase, so nothing of it
//                       depends on one prime per launch
//           conversion  hb_mixed_mont_kernel (hb_mixed.hpp) as it is: it reads
//                       obase and chunks of the PbProof entry and the record
//           sum         hb_cmixed_sum_kernel (here)
//   verify  PRF         hb_cmixed_prf_kernel (here): hb_cpv_prf_body with the
//                       alpha slot from the proof's item entry
//           sum         hb_vmixed_sum_kernel (hb_mixed.hpp) as it is, as the
//                       one-prime cxx verify uses hb_vbatch_sum_kernel
// The modulus is read through hb_table_ref (hb_mixed.hpp), never by value.
#pragma once
#include "hb_cpv.hpp"
#include "hb_mixed.hpp"
#include "hb_cmixed_args.hpp"

// hb_cpv_sum_kernel's body with the geometry, the modulus and the result
// column of the proof's record; one workgroup per entry of A.wgs.  A sector's
// offset is (u32)(idx C_f + j ss_f) with the proof's own C (cxx/
// shacham_waters_private.cxx:738, 762-763); a check_all proof takes block i as
// term i and reads no index.
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_cmixed_sum_kernel(CmSumArgs<NL> A) {
    __shared__ u32 sh[HB_WSUM_WG * (NL + 1)];
    MxWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    const u32 proof = __builtin_amdgcn_readfirstlane(W.proof), col = __builtin_amdgcn_readfirstlane(W.a);
    PbProof V;
    hb_load_uniform(A.proofs, proof, V);
    const MxRec<NL> &R = hb_table_ref(A.recs, proof);
    const u64 C = R.C;
    const u32 ss = R.ss, S = R.S, tw = R.tw;
    const u32 chunks = __builtin_amdgcn_readfirstlane(V.chunks);
    const u32 flags = __builtin_amdgcn_readfirstlane(V.flags);
    const bool load16 = (flags & HB_PB_LOAD16) != 0, all = (flags & HB_CMX_ALL) != 0;
    const u64 *idx = A.idx + V.obase;
    const u32 *vm = A.vm + V.obase * NL;
    u32 v[NL + 1], r[NL];
    {
        u32 acc[2 * NL + 1];
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        for (u32 i = threadIdx.x; i < chunks; i += HB_WSUM_WG) {
            const u64 blk = all ? (u64)i : idx[i];
            u32 m[NL];
            if (blk >= V.ntags) {   // (no stored index is: hb_cpv_prf_kernel stores 0 for one)
                for (int t = 0; t < NL; ++t) m[t] = 0;
            } else if (col < S) {
                const u64 pos = (u64)(u32)(blk * C + (u64)col * ss);
                if (load16) hb_sector_value<NL, 16>(V.data, V.len, pos, ss, m);
                else hb_sector_value<NL, 1>(V.data, V.len, pos, ss, m);
            } else if (load16) {
                hb_load_full16<NL>(V.tags, blk * tw, m);
            } else {
                hb_load_be_bytes<NL>(V.tags, blk * tw, tw, m);
            }
            hb_mac<NL>(acc, vm + (u64)i * NL, m);
        }
        hb_redc<NL>(acc, R.mod, v);
    }
    hb_reduce_small<NL>(v, R.mod, r);
    for (int t = 0; t < NL; ++t) sh[threadIdx.x * (NL + 1) + t] = r[t];
    sh[threadIdx.x * (NL + 1) + NL] = 0;
    __syncthreads();
    hb_tree_sum<NL>(sh, HB_WSUM_WG);
    if (threadIdx.x == 0) {
        for (int t = 0; t <= NL; ++t) v[t] = sh[t];
        hb_reduce_small<NL>(v, R.mod, r);
        u32 *res = A.res + ((u64)R.col0 + col) * NL;
        for (int t = 0; t < NL; ++t) res[t] = r[t];
    }
}

// Each proof's own first alpha slot (hb_cmixed_args.hpp: above the flag bit of
// the item's flags word), read through the table where it is used, as
// hb_cpv_prf_kernel reads S from the kernel arguments there: nothing more stays
// in a scalar register across the draw loop.
struct CmAlphaOwn {
    template <int NL>
    __device__ __forceinline__ u64 operator()(const CpvPrfArgs<NL> &A, u32 item) const {
        return (u64)(hb_table_ref(A.items, item).flags >> HB_CMX_SLOT_SHIFT);
    }
};

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_cmixed_prf_kernel(CpvPrfArgs<NL> A) {
    hb_cpv_prf_body<NL, NR>(A, CmAlphaOwn{});
}

template <int NL>
hipError_t hb_launch_cmixed_sum(const CmSumArgs<NL> &A, u32 nwg, hipStream_t s) {
    HB_LAUNCH((hb_cmixed_sum_kernel<NL>), dim3(nwg), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_cmixed_prf(const CpvPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_cmixed_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_cmixed_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_cmixed_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

#define HB_INST_CMIXED(NL)                                                                        \
    template hipError_t hb_launch_cmixed_sum<NL>(const CmSumArgs<NL> &, u32, hipStream_t);       \
    template hipError_t hb_launch_cmixed_prf<NL>(const CpvPrfArgs<NL> &, int, int, hipStream_t);
