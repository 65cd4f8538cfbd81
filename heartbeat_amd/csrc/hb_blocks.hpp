// hb_blocks.hpp -- the PRF kernel of the listed-block encode
// (hb_encode_blocks_many; instantiated by hb_kern_blocks.hip and
// hb_kern_blocks64.hip): F(indices[k]) of every listed block of every file and
// alpha_j of every file, each file under its own key schedules, in one launch.
//
// hb_batch_prf_kernel (hb_batch.hpp) with one difference: the F handler's PRF
// input is not the job number but the entry of the file's slice of a device
// index table -- a full 64-bit value, hashed as its decimal string of up to 20
// digits (hb_sha256_decimal).  A wave-job's first and count stay 32-bit: they
// count listed blocks, not indices.  The F values land where the batched
// encode's MAC kernels (hb_batch_mac_split_kernel, hb_batch_mac_kernel) read
// them, packed position by packed position, so the MAC launch follows on the
// stream with nothing in between.
#pragma once
#include "hb_batch.hpp"
#include "hb_blocks_args.hpp"

// BatchPrfHandler (hb_batch.hpp) whose F input comes from the index table
template <int NL>
struct BlocksPrfHandler {
    const BlocksPrfArgs<NL> &A;
    const u64 *idx;   // the file's slice of the index table (not read for alpha)
    u32 *out;         // the file's F values or alpha table
    bool alpha;
    __device__ __forceinline__ u64 x_of(u64 job) const { return alpha ? job : idx[job]; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void fail(u64) const {}
    __device__ __forceinline__ void accept(u64 job, const u32 v[NL]) const {
        u32 *o = out + job * NL;
        if (alpha) {
            u32 y[NL];
            hb_to_mont<NL>(v, A.r2, A.mod, y);
            hb_store_limbs<NL>(o, y);
        } else {
            hb_store_limbs<NL>(o, v);
        }
    }
};

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_blocks_prf_kernel(BlocksPrfArgs<NL> A) {
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
        BatchWaveJob J;
        hb_load_uniform(A.jobs, lo, J);
        const u32 file = __builtin_amdgcn_readfirstlane(J.file);
        const bool alpha = __builtin_amdgcn_readfirstlane(J.kind) != 0;
        const u32 first = __builtin_amdgcn_readfirstlane(J.first);
        const u32 count = __builtin_amdgcn_readfirstlane(J.count);
        PrfParams<NL> P;
        hb_load_uniform(A.prf, 2u * file + (alpha ? 1u : 0u), P);
        BatchFile F;
        hb_load_uniform(A.files, file, F);
        u32 *out = alpha ? A.amont + (u64)file * A.S * NL : A.fv + F.fbase * NL;
        BlocksPrfHandler<NL> h{A, A.idx + F.fbase, out, alpha};
        // placed jobs [first, first + count) of the file's list (alpha: of its
        // sectors): the engine never touches queue[0]
        hb_engine_quad<NL, NR, BlocksPrfHandler<NL>>(h, L, P, (u64)first + count, A.queue + (alpha ? HB_QSLOT : 0), 16,
                                                      (u64)first);
    }
}

template <int NL>
hipError_t hb_launch_blocks_prf(const BlocksPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_blocks_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_blocks_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_blocks_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

#define HB_INST_BLOCKS(NL) \
    template hipError_t hb_launch_blocks_prf<NL>(const BlocksPrfArgs<NL> &, int, int, hipStream_t);
