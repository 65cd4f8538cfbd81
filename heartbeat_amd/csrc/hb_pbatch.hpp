// hb_pbatch.hpp -- kernels of the batched prove (hb_prove_many; instantiated
// by hb_kern_pbatch.hip and hb_kern_pbatch64.hip): mu and sigma of many small
// proofs, each under its own challenge key, file and tag array, in one PRF
// launch and one sum launch.  Replaces a storage node's loop over
// heartbeat/PySwizzle/PySwizzle.py:333-370 (one hb_prove per challenge).
//
// A single prove of a small file is latency-bound like a single verify: its
// launch puts a few dozen quad-engine waves on a chip with 16 x #CUs wave
// positions and lasts as long as its longest rejection chain.
// hb_prove_prf_kernel takes the challenge key's two schedules from the kernel
// arguments, so N proofs are N launches in series.  Here, as in the batched
// verify (hb_vbatch.hpp), the schedules of all proofs are a device table and a
// wave picks the ones of the wave-job it took from the queue.  Nothing of the
// fused prove's LDS polling, counters or token is used: the PRF launch stores
// idx and v (raw limbs), hb_mont_kernel turns the group's v into Montgomery
// form, and the sum launch that follows in stream order reads both.
//
// Where v becomes v R mod p.  Neither factor of a term is below p here (v_i
// up to v_max, which may exceed p; a sector of bitlen(p) / 8 bytes exceeds p
// when bitlen(p) is a multiple of 8; tags are the caller's bytes), so the
// exact-accumulate-then-REDC sum needs v in Montgomery form (< p), as
// ProveVHandler and hb_wsum_kernel have it.  In the PRF kernel's accept the
// conversion's 2NL+1-limb product sits inside the engine's live state (the
// batched verify measured 340 B / 1,552 B of scratch at NL 32 / 64 for that,
// DESIGN.md 5.3b; here 324 B / 1,504 B); once per term in the
// sum kernel it is redone for each of the S + 1 columns, two thirds of that
// kernel's multiplies.  So it
// is a pass of its own over the group's contiguous v buffer, the existing
// hb_mont_kernel, in place: one thread per term, and both new kernels keep
// the register footprint of their verify counterparts.
//
// Queue order (the host writes it, prove_many_impl): longest wave-job first.
// A try of the v engine is bytes(v_max) CFB-8 steps, a try of the index engine
// bytes(ntags) <= 8, and both draw the same expected number of tries (below
// 2), so the v wave-jobs of every proof come first and the index wave-jobs
// after them whenever bytes(v_max) >= bytes(ntags) over the group -- always at
// PySwizzle's v_max = p -- and the other way round for a tiny v_max.  A free
// wave takes the next entry, so the launch ends on the shorter kind.
#pragma once
#include "hb_batch.hpp"
#include "hb_pbatch_args.hpp"

// idx_i as u64.  An abandoned job (counted: the call fails) still stores an
// in-range index, so that the sum launch never forms an address from a word
// this launch did not write.
struct PbIdxHandler {
    u64 *out;
    __device__ __forceinline__ u64 x_of(u64 job) const { return job; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void accept(u64 job, const u32 v[2]) const { out[job] = (u64)v[0] | ((u64)v[1] << 32); }
    __device__ __forceinline__ void fail(u64 job) const { out[job] = 0; }
};

// v_i, stored raw (see above)
template <int NL>
struct PbVHandler {
    u32 *out;
    __device__ __forceinline__ u64 x_of(u64 job) const { return job; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void fail(u64) const {}
    __device__ __forceinline__ void accept(u64 job, const u32 v[NL]) const { hb_store_limbs<NL>(out + job * NL, v); }
};

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_pbatch_prf_kernel(PbPrfArgs<NL> A) {
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
        PbWaveJob J;
        hb_load_uniform(A.jobs, lo, J);
        const u32 proof = __builtin_amdgcn_readfirstlane(J.proof);
        const u32 kind = __builtin_amdgcn_readfirstlane(J.kind);
        const u64 first = __builtin_amdgcn_readfirstlane(J.first);
        const u64 stop = first + __builtin_amdgcn_readfirstlane(J.count);
        PbProof V;
        hb_load_uniform(A.proofs, proof, V);
        // placed jobs [first, stop): the engines never touch queue[0]; tries
        // and abandoned jobs go to the kind's slot
        unsigned long long *q = A.queue + kind * HB_QSLOT;
        if (kind == HB_PB_IDX) {
            PrfParams<2> PI;
            hb_load_uniform(A.pidx, proof, PI);
            PbIdxHandler h{A.idx + V.obase};
            hb_engine_quad<2, NR, PbIdxHandler>(h, L, PI, stop, q, 16, first);
        } else {
            PrfParams<NL> P;
            hb_load_uniform(A.pv, proof, P);
            PbVHandler<NL> h{A.vv + V.obase * NL};
            hb_engine_quad<NL, NR, PbVHandler<NL>>(h, L, P, stop, q, 16, first);
        }
    }
}

// One (proof, column) result per workgroup: column j < S is mu_j = sum_i v_i *
// sector j of block idx_i (absolute offset idx_i C + j ss; hb_sector_value: a
// short last sector right-aligned, a sector past len 0), column S is sigma =
// sum_i v_i * tags[idx_i]  (PySwizzle.py:351-368).  Each thread adds its k
// products exactly (2NL+1 limbs; v_i R mod p < p, the other factor < 2^(32 NL),
// so each is < p 2^(32 NL)) and reduces once: REDC gives the sum mod p up to
// (k + 1) p, inside hb_reduce_small's 2^32 p.  The workgroup's residues are
// tree-summed (< 256 p) and reduced.  No cross-workgroup state.  A proof with
// HB_PB_LOAD16 (full-width sectors and tags, everything 16-byte aligned; the
// host decides per proof) reads whole sectors and tags with 16-byte loads: the
// byte loop of hb_load_be_bytes is 4 NL dependent loads and shifts per term,
// more than the term's multiply (DESIGN.md 5.3c has the A/B).
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_pbatch_sum_kernel(PbSumArgs<NL> A) {
    __shared__ u32 sh[HB_WSUM_WG * (NL + 1)];
    const u32 ncols = A.S + 1;
    const u32 proof = blockIdx.x / ncols, col = blockIdx.x % ncols;
    PbProof V;
    hb_load_uniform(A.proofs, proof, V);
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
            } else if (col < A.S) {
                const u64 pos = blk * A.C + (u64)col * A.ss;
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
hipError_t hb_launch_pbatch_prf(const PbPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_pbatch_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_pbatch_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_pbatch_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

// nproofs * (S + 1) workgroups
template <int NL>
hipError_t hb_launch_pbatch_sum(const PbSumArgs<NL> &A, u32 nwg, hipStream_t s) {
    HB_LAUNCH((hb_pbatch_sum_kernel<NL>), dim3(nwg), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

#define HB_INST_PBATCH(NL)                                                                        \
    template hipError_t hb_launch_pbatch_prf<NL>(const PbPrfArgs<NL> &, int, int, hipStream_t);  \
    template hipError_t hb_launch_pbatch_sum<NL>(const PbSumArgs<NL> &, u32, hipStream_t);
