// hb_vbatch.hpp -- kernels of the batched verify (hb_verify_rhs_many;
// instantiated by hb_kern_vbatch.hip and hb_kern_vbatch64.hip): the right-hand
// sides of many small proofs, each under its own f_key, alpha_key and challenge
// key, in one PRF launch and one sum launch.
//
// A single verify is latency-bound like a small encode: its fused launch puts
// a few dozen quad-engine waves on a chip with 16 x #CUs wave positions and
// lasts as long as its longest rejection chain.  The fused
// kernel takes its four key schedules from the kernel arguments, so N proofs
// are N launches in series.  Here, as in the batched encode (hb_batch.hpp),
// the schedules of all proofs are a device table and a wave picks the ones of
// the wave-job it took from the queue.  Nothing of the fused kernels' LDS
// polling, counters or token is used: the PRF launch stores v, F and alpha
// (raw limbs), the sum launch that follows it in stream order reads them.
//
// Queue order (the host writes it, verify_many_impl): every proof's index + F
// wave-jobs first, then every proof's alpha wave-jobs, then every proof's v
// wave-jobs.  A free wave takes the next entry, so this is longest job first:
// an index + F job runs two engines in a row (up to 8 index bytes per try,
// then bytes(p) per try), alpha tries are bytes(p) long, v tries bytes(v_max)
// <= 4 NL.  With the proofs' kinds interleaved as in the batched encode, the
// last proof's two-engine chains would start when the queue is nearly drained
// and the launch would end on them alone; in this order the launch ends on the
// shortest kind.
#pragma once
#include "hb_batch.hpp"
#include "hb_vbatch_args.hpp"

// idx_i into the wave's 16 LDS slots (see the hand-over note in the kernel)
struct VbIdxHandler {
    u64 *slot;
    u64 first;
    __device__ __forceinline__ u64 x_of(u64 job) const { return job; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void accept(u64 job, const u32 v[2]) const {
        slot[job - first] = (u64)v[0] | ((u64)v[1] << 32);
    }
    __device__ __forceinline__ void fail(u64 job) const { slot[job - first] = 0; }   // counted: the call fails
};

// The wave-job's NL-limb engine: F(idx_i) (PySwizzle.py:389; the input is the
// slot's index), v_i or alpha_j (the input is the job's number), all stored
// raw -- the sum kernel takes the Montgomery factor out once per thread, so
// this kernel holds no conversion (hb_to_mont's 2NL+1-limb product is what
// spills in hb_batch_prf_kernel at NL >= 32).  `idxf` is wave-uniform.
template <int NL>
struct VbHandler {
    const u64 *slot;
    u64 first;
    u32 *out;       // the proof's F values, v values or alpha table
    bool idxf;
    __device__ __forceinline__ u64 x_of(u64 job) const { return idxf ? slot[job - first] : job; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void fail(u64) const {}
    __device__ __forceinline__ void accept(u64 job, const u32 v[NL]) const { hb_store_limbs<NL>(out + job * NL, v); }
};

// Where a proof's alpha values land in A.av, in slots of NL limbs: with one S
// for the batch, proof * S.  (hb_mixed.hpp has the other one: each proof's
// own first slot, from its record.)
struct VbAlphaShared {
    u32 S;
    __device__ __forceinline__ u64 operator()(u32 proof) const { return (u64)proof * S; }
};

// The PRF launch's body, shared by hb_vbatch_prf_kernel and the mixed-owner
// batch's hb_vmixed_prf_kernel: they differ in AlphaBase alone.
template <int NL, int NR, class AlphaBase>
__device__ __forceinline__ void hb_vbatch_prf_body(const VbPrfArgs<NL> &A, const AlphaBase &alpha_base) {
    __shared__ __attribute__((aligned(16))) u32 lds[HB_LDS_WORDS];
    __shared__ u64 xidx[HB_ENGINE_WG / 64][16];
    hb_fill_lds(lds, A.t0);
    const LaneTab L = hb_lane_tab(lds);
    u64 *slot = xidx[threadIdx.x >> 6];
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
        VbWaveJob J;
        hb_load_uniform(A.jobs, lo, J);
        const u32 proof = __builtin_amdgcn_readfirstlane(J.proof);
        const u32 kind = __builtin_amdgcn_readfirstlane(J.kind);
        const u64 first = __builtin_amdgcn_readfirstlane(J.first);
        const u64 stop = first + __builtin_amdgcn_readfirstlane(J.count);
        VbProof V;
        hb_load_uniform(A.proofs, proof, V);
        // placed jobs [first, stop): the engines never touch queue[0]; tries
        // and abandoned jobs go to the kind's slot
        unsigned long long *q = A.queue + kind * HB_QSLOT;
        const bool idxf = kind == HB_VB_IDXF;
        if (idxf) {
            PrfParams<2> PI;
            hb_load_uniform(A.pidx, proof, PI);
            VbIdxHandler hi2{slot, first};
            hb_engine_quad<2, NR, VbIdxHandler>(hi2, L, PI, stop, q, 16, first);
            // Hand-over of the 16 indices inside the wave: the lead lane of a
            // quad stored its index into this wave's LDS slots (accept), all
            // four lanes of a quad read it in the F engine (x_of).  LDS
            // executes one wave's instructions in issue order, so the reads
            // see the writes once the compiler keeps them in program order:
            // the release / acquire fence pair at workgroup scope does that
            // (and waits for the LDS counter); no cache is involved.  The
            // slots are this wave's own, and the next index engine of this
            // wave writes them only after this job's F engine has read them
            // (the lead lane's own read precedes its next write).
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        PrfParams<NL> P;
        hb_load_uniform(A.prf, 3u * proof + kind, P);
        u32 *out = kind == HB_VB_ALPHA ? A.av + alpha_base(proof) * NL : (idxf ? A.fv : A.vv) + V.obase * NL;
        VbHandler<NL> h{slot, first, out, idxf};
        hb_engine_quad<NL, NR, VbHandler<NL>>(h, L, P, stop, q, 16, first);
    }
}

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_vbatch_prf_kernel(VbPrfArgs<NL> A) {
    hb_vbatch_prf_body<NL, NR>(A, VbAlphaShared{A.S});
}

// rhs of one proof per workgroup: sum_i v_i F_i + sum_j alpha_j mu_j mod p
// over raw factors.  Each thread adds its k products exactly (2NL+1 limbs;
// one factor of every product is < p -- F_i, alpha_j -- the other < 2^(32 NL),
// so each is < p 2^(32 NL)) and reduces once: REDC gives sum / R mod p
// (< (k + 1) p, inside hb_reduce_small's 2^32 p), and hb_to_mont of that
// residue -- times R^2, REDC -- gives the sum mod p.  The workgroup's residues
// are tree-summed (< 256 p) and reduced.  No cross-workgroup state.
template <int NL>
__global__ __launch_bounds__(HB_WSUM_WG) void hb_vbatch_sum_kernel(VbSumArgs<NL> A) {
    __shared__ u32 sh[HB_WSUM_WG * (NL + 1)];
    const u32 proof = blockIdx.x;
    VbProof V;
    hb_load_uniform(A.proofs, proof, V);
    const u32 chunks = __builtin_amdgcn_readfirstlane(V.chunks);
    const u32 *vv = A.vv + V.obase * NL, *fv = A.fv + V.obase * NL;
    const u32 *av = A.av + (u64)proof * A.S * NL, *mu = A.mu + (u64)proof * A.S * NL;
    const u32 nterms = chunks + A.S;
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
        hb_redc<NL>(acc, A.mod, v);
    }
    hb_reduce_small<NL>(v, A.mod, r);
    if (threadIdx.x < nterms) {   // (the others hold 0)
        u32 y[NL];
        hb_to_mont<NL>(r, A.r2, A.mod, y);
        for (int t = 0; t < NL; ++t) r[t] = y[t];
    }
    for (int t = 0; t < NL; ++t) sh[threadIdx.x * (NL + 1) + t] = r[t];
    sh[threadIdx.x * (NL + 1) + NL] = 0;
    __syncthreads();
    hb_tree_sum<NL>(sh, HB_WSUM_WG);
    if (threadIdx.x == 0) {
        for (int t = 0; t <= NL; ++t) v[t] = sh[t];
        hb_reduce_small<NL>(v, A.mod, r);
        for (int t = 0; t < NL; ++t) A.res[(u64)proof * NL + t] = r[t];
    }
}

template <int NL>
hipError_t hb_launch_vbatch_prf(const VbPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_vbatch_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_vbatch_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_vbatch_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_vbatch_sum(const VbSumArgs<NL> &A, u32 nproofs, hipStream_t s) {
    HB_LAUNCH((hb_vbatch_sum_kernel<NL>), dim3(nproofs), dim3(HB_WSUM_WG), s, A);
    return hipGetLastError();
}

#define HB_INST_VBATCH(NL)                                                                        \
    template hipError_t hb_launch_vbatch_prf<NL>(const VbPrfArgs<NL> &, int, int, hipStream_t);  \
    template hipError_t hb_launch_vbatch_sum<NL>(const VbSumArgs<NL> &, u32, hipStream_t);
