// hb_mixed.hpp -- kernels of the mixed-owner batches (hb_prove_mixed,
// hb_verify_rhs_mixed; instantiated by hb_kern_mixed.hip and
// hb_kern_mixed64.hip): the batched prove and verify of hb_pbatch.hpp and
// hb_vbatch.hpp for proofs that each name their own prime and sector count.
// Replaces a storage node's loop of hb_prove over the challenges of many
// owners (heartbeat/PySwizzle/PySwizzle.py:333-370 per proof, one prime per
// PySwizzle instance, :250-251) and an auditor's loop of hb_verify_rhs
// (:381-394).
//
// The PRF launches need nothing of the prime that is not in the schedules
// already: hb_pbatch_prf_kernel is used as it is, hb_vbatch_prf_kernel's body
// with the alpha slot from the proof's record.  What takes the modulus is the
// conversion v -> v R mod p and the two sum kernels.  There the one-prime
// kernels read ModP and R^2 from the kernel arguments (scalar loads where
// they are used); here they are a record per proof (MxRec) and a kernel reads
// them through hb_table_ref: a wave-uniform reference into the table in the
// constant address space, so that hb_redc / hb_reduce_small / hb_to_mont load
// p's limbs with scalar loads at their use, exactly as from the kernel
// arguments.  A by-value copy of a record would be up to 2 NL + 12 words per
// lane (DESIGN.md 5.3g has the resource usage of both forms' kernels).
//
// The conversion stays a pass of its own (hb_pbatch.hpp: why).  Its
// workgroups do not straddle proofs: workgroup w takes the (proof, first
// term) entry w of a table and converts up to 256 terms of that proof, so the
// modulus is uniform over the workgroup and the last workgroup of a proof is
// partly idle (at most 255 lanes per proof, against a second table lookup per
// lane).
#pragma once
#include "hb_pbatch.hpp"
#include "hb_vbatch.hpp"
#include "hb_mixed_args.hpp"

// tab[idx] by reference for a wave-uniform idx of a table the host wrote
// before the launch: loads through it are scalar loads (see hb_load_uniform).
template <class T>
__device__ __forceinline__ const T &hb_table_ref(const T *tab, u32 idx) {
    typedef const T __attribute__((address_space(4))) *cptr;
    return *(const T *)(cptr)(uintptr_t)(tab + idx);
}

template <int NL>
__global__ __launch_bounds__(HB_MX_MONT_WG) void hb_mixed_mont_kernel(MxMontArgs<NL> A) {
    MxWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    const u32 proof = __builtin_amdgcn_readfirstlane(W.proof);
    PbProof V;
    hb_load_uniform(A.proofs, proof, V);
    const u32 i = __builtin_amdgcn_readfirstlane(W.a) + threadIdx.x;
    if (i >= V.chunks) return;
    const MxRec<NL> &R = hb_table_ref(A.recs, proof);
    u32 *at = A.vv + (V.obase + i) * NL;
    u32 x[NL], y[NL];
    for (int t = 0; t < NL; ++t) x[t] = at[t];
    hb_to_mont<NL>(x, R.r2, R.mod, y);
    for (int t = 0; t < NL; ++t) at[t] = y[t];
}

// hb_pbatch_sum_kernel's body with the geometry, the modulus and the result
// column of the proof's record; one workgroup per entry of A.wgs.
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_mixed_sum_kernel(MxSumArgs<NL> A) {
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
    const bool load16 = (__builtin_amdgcn_readfirstlane(V.flags) & HB_PB_LOAD16) != 0;
    const u64 *idx = A.idx + V.obase;
    const u32 *vm = A.vm + V.obase * NL;
    u32 v[NL + 1], r[NL];
    {
        u32 acc[2 * NL + 1];
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        for (u32 i = threadIdx.x; i < chunks; i += HB_WSUM_WG) {
            const u64 blk = idx[i];
            u32 m[NL];
            if (blk >= V.ntags) {   // (no stored index is: the PRF's range is ntags)
                for (int t = 0; t < NL; ++t) m[t] = 0;
            } else if (col < S) {
                const u64 pos = blk * C + (u64)col * ss;
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

// each proof's own first alpha slot
template <int NL>
struct VmAlphaOwn {
    const MxRec<NL> *recs;
    __device__ __forceinline__ u64 operator()(u32 proof) const { return hb_table_ref(recs, proof).slot0; }
};

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_vmixed_prf_kernel(VmPrfArgs<NL> A) {
    hb_vbatch_prf_body<NL, NR>(A.b, VmAlphaOwn<NL>{A.recs});
}

// hb_vbatch_sum_kernel's body with S, the alpha / mu slot, the modulus and R^2
// of the proof's record; one workgroup per proof.
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_vmixed_sum_kernel(VmSumArgs<NL> A) {
    __shared__ u32 sh[HB_WSUM_WG * (NL + 1)];
    const u32 proof = blockIdx.x;
    VbProof V;
    hb_load_uniform(A.proofs, proof, V);
    const MxRec<NL> &R = hb_table_ref(A.recs, proof);
    const u32 S = R.S;
    const u64 slot0 = R.slot0;
    const u32 chunks = __builtin_amdgcn_readfirstlane(V.chunks);
    const u32 *vv = A.vv + V.obase * NL, *fv = A.fv + V.obase * NL;
    const u32 *av = A.av + slot0 * NL, *mu = A.mu + slot0 * NL;
    const u32 nterms = chunks + S;
    u32 v[NL + 1], r[NL];
    {
        u32 acc[2 * NL + 1];
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        for (u32 i = threadIdx.x; i < nterms; i += HB_WSUM_WG) {
            const bool c = i < chunks;
            const u32 *w = c ? fv + (u64)i * NL : av + (u64)(i - chunks) * NL;   // the factor < p
            const u32 *x = c ? vv + (u64)i * NL : mu + (u64)(i - chunks) * NL;
            u32 m[NL];
            for (int t = 0; t < NL; ++t) m[t] = x[t];
            hb_mac<NL>(acc, w, m);
        }
        hb_redc<NL>(acc, R.mod, v);
    }
    hb_reduce_small<NL>(v, R.mod, r);
    if (threadIdx.x < nterms) {   // (the others hold 0)
        u32 y[NL];
        hb_to_mont<NL>(r, R.r2, R.mod, y);
        for (int t = 0; t < NL; ++t) r[t] = y[t];
    }
    for (int t = 0; t < NL; ++t) sh[threadIdx.x * (NL + 1) + t] = r[t];
    sh[threadIdx.x * (NL + 1) + NL] = 0;
    __syncthreads();
    hb_tree_sum<NL>(sh, HB_WSUM_WG);
    if (threadIdx.x == 0) {
        for (int t = 0; t <= NL; ++t) v[t] = sh[t];
        hb_reduce_small<NL>(v, R.mod, r);
        for (int t = 0; t < NL; ++t) A.res[(u64)proof * NL + t] = r[t];
    }
}

template <int NL>
hipError_t hb_launch_mixed_mont(const MxMontArgs<NL> &A, u32 nwg, hipStream_t s) {
    HB_LAUNCH((hb_mixed_mont_kernel<NL>), dim3(nwg), dim3(HB_MX_MONT_WG), s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_mixed_sum(const MxSumArgs<NL> &A, u32 nwg, hipStream_t s) {
    HB_LAUNCH((hb_mixed_sum_kernel<NL>), dim3(nwg), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_vmixed_prf(const VmPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_vmixed_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_vmixed_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_vmixed_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_vmixed_sum(const VmSumArgs<NL> &A, u32 nproofs, hipStream_t s) {
    HB_LAUNCH((hb_vmixed_sum_kernel<NL>), dim3(nproofs), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

#define HB_INST_MIXED(NL)                                                                         \
    template hipError_t hb_launch_mixed_mont<NL>(const MxMontArgs<NL> &, u32, hipStream_t);      \
    template hipError_t hb_launch_mixed_sum<NL>(const MxSumArgs<NL> &, u32, hipStream_t);        \
    template hipError_t hb_launch_vmixed_prf<NL>(const VmPrfArgs<NL> &, int, int, hipStream_t);  \
    template hipError_t hb_launch_vmixed_sum<NL>(const VmSumArgs<NL> &, u32, hipStream_t);
