// hb_cpv.hpp -- kernels of the batched cxx prove and verify (hb_cxx_prove_many,
// hb_cxx_verify_rhs_many; instantiated by hb_kern_cpv.hip and
// hb_kern_cpv64.hip): the proofs of many small files of the cxx Swizzle, each
// under its own keys, in one PRF launch and one sum launch per group.
// Replaces a storage node's loop over cxx/shacham_waters_private.cxx:731-789
// (one hb_prove with HB_PRF_CXX per challenge) and an auditor's loop over
// :791-842 (one hb_cxx_verify_rhs per proof), both with the cxx prf
// (cxx/prf.hxx:125-176).
//
// The PRF launch is hb_cbatch_prf_kernel's (hb_cbatch.hpp): 1,024-thread
// workgroups that fill the LDS T-table image, one atomic on queue slot 0 per
// wave-job, the job, the item entry and the key schedule read with scalar
// loads, one lane per evaluation, a wave-job of at most HB_CB_JOB evaluations
// of one item under one key.  The lane functions are the single calls'
// (hb_sha256_le32, hb_cxx_try, hb_cxx_try_bytes), so the 81-try rule has one
// place.  Kinds (hb_cbatch_plan.hpp):
//   HB_CB_V      v_i = prf(chal_key, v_max)(i), raw limbs (hb_mont_kernel
//                follows for a prove; the verify sum takes raw factors)
//   HB_CB_IDX    idx_i = prf(chal_key, ntags)(i) as u64 (prove, sampled).  The
//                limit's ByteCount is 1..8 and never a multiple of 16: the
//                byte-granular continuation hb_cxx_try_bytes on PrfParams<2>.
//                An index the forced accept leaves >= ntags is stored as 0 and
//                flagged in the item's status word, so the sum launch never
//                forms an address from it (the reference's
//                t.sigma().at(index) throws there).
//   HB_CB_IDXF   the lane draws idx_i the same way and evaluates F(idx_i) =
//                prf(f_key, p)(idx_i) under the F schedule; with check_all it
//                evaluates F(i).  The index never reaches memory, and any
//                index is taken (verify has no range check, :829-833).
//   HB_CB_ALPHA  alpha_j = prf(alpha_key, p)(j), raw limbs
// Every loop is bounded by the wave-job's count x 81 tries; no workgroup waits
// for another.
#pragma once
#include "hb_batch.hpp"
#include "hb_cpv_args.hpp"

// Where an item's alpha values land in A.av, in slots of NL limbs: with one S
// for the batch, item * S.  (hb_cmixed.hpp has the other one: each proof's
// own first slot, read from the item's entry where it is used.)
struct CpvAlphaShared {
    u32 S;
    template <int NL>
    __device__ __forceinline__ u64 operator()(const CpvPrfArgs<NL> &, u32 item) const { return (u64)item * S; }
};

// The PRF launch's body, shared by hb_cpv_prf_kernel and the cxx mixed-owner
// batch's hb_cmixed_prf_kernel: they differ in AlphaBase alone.
template <int NL, int NR, class AlphaBase>
__device__ __forceinline__ void hb_cpv_prf_body(const CpvPrfArgs<NL> &A, const AlphaBase &alpha_base) {
    __shared__ __attribute__((aligned(16))) u32 lds[HB_LDS_WORDS];
    hb_fill_lds(lds, A.t0);
    const LaneTab L = hb_lane_tab(lds);
    for (;;) {
        u32 lo = 0, hi = 0;
        if (hb_lane_id() == 0) {
            const u64 t = atomicAdd(A.queue, 1ull);
            lo = (u32)t;
            hi = (u32)(t >> 32);
        }
        lo = __builtin_amdgcn_readfirstlane(lo);
        hi = __builtin_amdgcn_readfirstlane(hi);
        if (hi || (u64)lo >= A.njobs) break;
        HbCbJob J;
        hb_load_uniform(A.jobs, lo, J);
        const u32 item = __builtin_amdgcn_readfirstlane(J.item);
        const u32 kind = __builtin_amdgcn_readfirstlane(J.kind);
        const u32 first = __builtin_amdgcn_readfirstlane(J.first);
        const u32 stop = first + __builtin_amdgcn_readfirstlane(J.count);
        CpvItem V;
        hb_load_uniform(A.items, item, V);
        const bool all = (__builtin_amdgcn_readfirstlane(V.flags) & HB_CPV_ALL) != 0;
        const bool draw = kind == HB_CB_IDX || (kind == HB_CB_IDXF && !all);
        u32 tries = 0;
        // 64 evaluations at a time, one per lane (HB_CB_JOB = 64: one pass)
        for (u32 base = first; base < stop; base += 64u) {
            const u32 i = base + hb_lane_id();
            const bool live = i < stop;
            u64 x = i;
            u32 dig[8], sr[4] = {0, 0, 0, 0};
            if (draw) {
                PrfParams<2> PI;
                hb_load_uniform(A.pidx, item, PI);
                u32 o[2];
                hb_sha256_le32(i, dig);
                bool active = live;
                u32 job_tries = 0;
                while (__ballot(active)) {
                    u32 ok = hb_cxx_try_bytes<2, NR>(L, PI, sr, dig, o, job_tries);
                    tries += active ? 1u : 0u;
                    job_tries += 1u;
                    if (job_tries >= HB_CXX_MAX_TRIES) ok = 1;   // `count++ < 80` (prf.hxx:142)
                    if (active && ok) {
                        x = (u64)o[0] | ((u64)o[1] << 32);
                        active = false;
                    }
                }
            }
            if (kind == HB_CB_IDX) {
                if (live) {
                    if (x >= V.range) {
                        x = 0;
                        atomicOr(A.status + item, 1u);
                    }
                    A.idx[V.obase + i] = x;
                }
                continue;
            }
            const u32 slot = kind == HB_CB_V ? HB_CPV_PV : kind == HB_CB_IDXF ? HB_CPV_PF : HB_CPV_PA;
            PrfParams<NL> P;
            hb_load_uniform(A.prf, A.stride * item + slot, P);
            u32 *dst = kind == HB_CB_V      ? A.vv + (V.obase + i) * NL
                       : kind == HB_CB_IDXF ? A.fv + (V.obase + i) * NL
                                            : A.av + (alpha_base(A, item) + i) * NL;
            u32 out[NL];
            hb_zero_sr(sr);   // resynchronised per evaluate (prf.hxx:132)
            hb_sha256_le32((u32)x, dig);
            bool active = live;
            u32 job_tries = 0;
            while (__ballot(active)) {
                u32 ok = hb_cxx_try<NL, NR>(L, P, sr, dig, out);
                tries += active ? 1u : 0u;
                job_tries += 1u;
                if (job_tries >= HB_CXX_MAX_TRIES) ok = 1;
                if (active && ok) {
                    hb_store_limbs<NL>(dst, out);
                    active = false;
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) tries += __shfl_xor(tries, off);
        if (hb_lane_id() == 0 && tries) atomicAdd(A.queue + kind * HB_QSLOT + 1, (unsigned long long)tries);
    }
}

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_cpv_prf_kernel(CpvPrfArgs<NL> A) {
    hb_cpv_prf_body<NL, NR>(A, CpvAlphaShared{A.S});
}

// One (file, column) result per workgroup, hb_pbatch_sum_kernel's sum with the
// cxx prove's two differences: a check_all file takes block i as term i (no
// index buffer), and a sector's offset is computed in unsigned int
// (cxx/shacham_waters_private.cxx:738, 762-763), so a file past 4 GiB reads
// sector j of block idx at (u32)(idx C + j ss).  Tags are indexed in full
// width (t.sigma().at(index)).  The bounds of each thread's exact sum are
// hb_pbatch_sum_kernel's.
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_cpv_sum_kernel(CpvSumArgs<NL> A) {
    __shared__ u32 sh[HB_WSUM_WG * (NL + 1)];
    const u32 ncols = A.S + 1;
    const u32 file = blockIdx.x / ncols, col = blockIdx.x % ncols;
    CpvFile V;
    hb_load_uniform(A.files, file, V);
    const u32 chunks = __builtin_amdgcn_readfirstlane(V.chunks);
    const u32 flags = __builtin_amdgcn_readfirstlane(V.flags);
    const bool load16 = (flags & HB_CPV_LOAD16) != 0, all = (flags & HB_CPV_ALL) != 0;
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
            } else if (col < A.S) {
                const u64 pos = (u64)(u32)(blk * A.C + (u64)col * A.ss);
                if (load16) hb_sector_value<NL, 16>(V.data, V.len, pos, A.ss, m);
                else hb_sector_value<NL, 1>(V.data, V.len, pos, A.ss, m);
            } else if (load16) {
                hb_load_full16<NL>(V.tags, blk * A.tw, m);
            } else {
                hb_load_be_bytes<NL>(V.tags, blk * A.tw, A.tw, m);
            }
            hb_mac<NL>(acc, vm + (u64)i * NL, m);
        }
        hb_redc<NL>(acc, A.mod, v);
    }
    hb_reduce_small<NL>(v, A.mod, r);
    for (int t = 0; t < NL; ++t) sh[threadIdx.x * (NL + 1) + t] = r[t];
    sh[threadIdx.x * (NL + 1) + NL] = 0;
    __syncthreads();
    hb_tree_sum<NL>(sh, HB_WSUM_WG);
    if (threadIdx.x == 0) {
        for (int t = 0; t <= NL; ++t) v[t] = sh[t];
        hb_reduce_small<NL>(v, A.mod, r);
        for (int t = 0; t < NL; ++t) A.res[(u64)blockIdx.x * NL + t] = r[t];
    }
}

template <int NL>
hipError_t hb_launch_cpv_prf(const CpvPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_cpv_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_cpv_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_cpv_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

// nfiles * (S + 1) workgroups
template <int NL>
hipError_t hb_launch_cpv_sum(const CpvSumArgs<NL> &A, u32 nwg, hipStream_t s) {
    HB_LAUNCH((hb_cpv_sum_kernel<NL>), dim3(nwg), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

#define HB_INST_CPV(NL)                                                                        \
    template hipError_t hb_launch_cpv_prf<NL>(const CpvPrfArgs<NL> &, int, int, hipStream_t); \
    template hipError_t hb_launch_cpv_sum<NL>(const CpvSumArgs<NL> &, u32, hipStream_t);
