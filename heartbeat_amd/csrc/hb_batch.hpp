// hb_batch.hpp -- kernels of the batched encode (hb_encode_many; instantiated
// by hb_kern_batch.hip and hb_kern_batch64.hip): many small files, each under its own
// f_key and alpha_key, in one PRF launch and one MAC launch.
//
// A small file is latency-bound: its PRF launch lasts as long as its longest
// rejection chain while a few hundred quad-engine waves sit on a chip with
// 16 x #CUs wave positions.  Every other engine takes its key
// schedule from the kernel arguments, one per launch; here the schedules of
// all files are a device table, and a wave picks the one of the wave-job it
// took from the queue.
#pragma once
#include "hb_kernels.hpp"

// Wave-uniform loads of a table entry as scalar loads: the tables are written
// by the host before the launch and only read by it, so they may be read
// through the constant address space, whose loads at a uniform address are
// s_load.  (A per-lane copy of a PrfParams would be 74 + NL VGPRs or scratch:
// see the note at hb_engine_quad.)
typedef const u32 __attribute__((address_space(4))) *hb_cu32;

template <class T>
__device__ __forceinline__ void hb_load_uniform(const T *tab, u32 idx, T &out) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    hb_cu32 s = (hb_cu32)(uintptr_t)(tab + idx);
    u32 *d = reinterpret_cast<u32 *>(&out);
    HB_UNROLL
    for (u32 i = 0; i < sizeof(T) / 4; ++i) d[i] = s[i];
}

// F(k) as limbs into the batch's F buffer, alpha_j in Montgomery form into the
// file's alpha table (PrfHandler / AlphaMontHandler with a wave-uniform target).
template <int NL>
struct BatchPrfHandler {
    const BatchPrfArgs<NL> &A;
    u32 *out;       // the file's F values or alpha table
    bool alpha;
    __device__ __forceinline__ u64 x_of(u64 job) const { return job; }
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
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_batch_prf_kernel(BatchPrfArgs<NL> A) {
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
        BatchPrfHandler<NL> h{A, out, alpha};
        // placed jobs [first, first + count): the engine never touches
        // queue[0]; tries and abandoned jobs go to the kind's slot
        hb_engine_quad<NL, NR, BatchPrfHandler<NL>>(h, L, P, (u64)first + count, A.queue + (alpha ? HB_QSLOT : 0), 16,
                                                     (u64)first);
    }
}

// tw big-endian bytes at any address
template <int NL>
__device__ __forceinline__ void hb_store_be_bytes(unsigned char *dst, u32 tw, const u32 v[NL]) {
    HB_UNROLL
    for (int t = 0; t < NL; ++t)
        HB_UNROLL
        for (int b = 0; b < 4; ++b) {
            const u32 pos = 4u * (u32)t + (u32)b;
            if (pos < tw) dst[tw - 1 - pos] = (unsigned char)(v[t] >> (8 * b));
        }
}

template <int NL>
__device__ __forceinline__ void hb_batch_store_tag(const BatchFile &F, u64 k, u32 tw, const u32 tag[NL]) {
    unsigned char *dst = F.tags + k * (u64)tw;
    if (F.flags & HB_BF_TAGS4) hb_store_be<NL>(dst, tw, tag);
    else hb_store_be_bytes<NL>(dst, tw, tag);
}

// hb_mac_split_kernel (2 <= S <= T) over the files of a batch: workgroup w
// takes blocks [first, first + T / S) of file wgs[w].file, lane (k, j) sector j
// of block k.  Sector values as everywhere: BE(data[off, min(off + ss, len))),
// 0 past the end of the file.
template <int NL>
__global__ __launch_bounds__(HbMacSplit<NL>::T) void hb_batch_mac_split_kernel(BatchMacArgs<NL> A) {
    constexpr int T = HbMacSplit<NL>::T;
    __shared__ u32 red[T * NL];
    BatchMacWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    BatchFile F;
    hb_load_uniform(A.files, W.file, F);
    const u32 S = A.S, bpw = T / S;
    const u32 lb = threadIdx.x / S, j = threadIdx.x % S;
    const u64 k = (u64)W.first + lb;
    const bool live = lb < bpw && k < F.nblocks;
    const u32 *fv = A.fv + (F.fbase + k) * NL;
    const u32 *am = A.amont + ((u64)W.file * S + j) * NL;
    if (live) {
        u32 acc[2 * NL + 1], m[NL];
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        if (j == 0)
            for (int t = 0; t < NL; ++t) acc[NL + t] = fv[t];
        const u64 off = k * A.C + (u64)j * A.ss;
        if (off < F.len) {
            const u32 r = (u32)(F.len - off < A.ss ? F.len - off : A.ss);
            if ((F.flags & HB_BF_LOAD16) && r == A.ss) hb_load_full16<NL>(F.data, off, m);
            else hb_load_be_bytes<NL>(F.data, off, r, m);
            hb_mac<NL>(acc, am, m);
        }
        u32 v[NL + 1], res[NL];
        hb_redc<NL>(acc, A.mod, v);
        hb_reduce_small<NL>(v, A.mod, res);
        for (int t = 0; t < NL; ++t) red[threadIdx.x * NL + t] = res[t];
    }
    __syncthreads();
    if (!live || j != 0) return;
    u32 v[NL + 1], tag[NL];
    u64 c = 0;
    for (int t = 0; t < NL; ++t) {   // S residues < p: the sum < S p < 2^32 p
        c += red[threadIdx.x * NL + t];
        for (u32 i = 1; i < S; ++i) c += red[(threadIdx.x + i) * NL + t];
        v[t] = (u32)c;
        c >>= 32;
    }
    v[NL] = (u32)c;
    hb_reduce_small<NL>(v, A.mod, tag);
    hb_batch_store_tag<NL>(F, k, A.tw, tag);
}

// hb_mac_kernel (S = 1 or S > T) over the files of a batch: one lane per block,
// workgroup w takes blocks [first, first + 256) of file wgs[w].file.
template <int NL>
__global__ __launch_bounds__(256) void hb_batch_mac_kernel(BatchMacArgs<NL> A) {
    BatchMacWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    BatchFile F;
    hb_load_uniform(A.files, W.file, F);
    const u64 k = (u64)W.first + threadIdx.x;
    if (k >= F.nblocks) return;
    u32 Fv[NL], tag[NL];
    for (int t = 0; t < NL; ++t) Fv[t] = A.fv[(F.fbase + k) * NL + t];
    const u32 *am = A.amont + (u64)W.file * A.S * NL;
    if (F.flags & HB_BF_LOAD16) hb_block_tag<NL, 16>(F.data, F.len, k, A.C, A.ss, A.S, am, A.mod, Fv, tag);
    else hb_block_tag<NL, 1>(F.data, F.len, k, A.C, A.ss, A.S, am, A.mod, Fv, tag);
    hb_batch_store_tag<NL>(F, k, A.tw, tag);
}

template <int NL>
hipError_t hb_launch_batch_prf(const BatchPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_batch_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_batch_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_batch_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

// Blocks per workgroup of the MAC launch for S sectors (the host builds the
// workgroup table with it)
template <int NL>
u32 hb_batch_mac_bpw(u32 S) {
    constexpr u32 T = HbMacSplit<NL>::T;
    return S >= 2 && S <= T ? T / S : 256u;
}

template <int NL>
hipError_t hb_launch_batch_mac(const BatchMacArgs<NL> &A, u32 nwg, hipStream_t s) {
    constexpr u32 T = HbMacSplit<NL>::T;
    if (hb_load_only) {
        hb_load_kernel(&hb_batch_mac_split_kernel<NL>);
        hb_load_kernel(&hb_batch_mac_kernel<NL>);
        return hipGetLastError();
    }
    if (A.S >= 2 && A.S <= T) HB_LAUNCH((hb_batch_mac_split_kernel<NL>), dim3(nwg), dim3((T / A.S) * A.S), s, A);
    else HB_LAUNCH((hb_batch_mac_kernel<NL>), dim3(nwg), dim3(256), s, A);
    return hipGetLastError();
}

#define HB_INST_BATCH(NL)                                                                        \
    template hipError_t hb_launch_batch_prf<NL>(const BatchPrfArgs<NL> &, int, int, hipStream_t); \
    template u32 hb_batch_mac_bpw<NL>(u32);                                                      \
    template hipError_t hb_launch_batch_mac<NL>(const BatchMacArgs<NL> &, u32, hipStream_t);
