// hb_emixed.hpp -- kernels of the mixed-owner encodes (hb_encode_mixed,
// hb_cxx_encode_mixed; instantiated by hb_kern_emixed.hip and
// hb_kern_emixed64.hip): the batched encodes of hb_batch.hpp and hb_cbatch.hpp
// for files that each name their own prime and sector count.  Replaces a loop
// of single encodes over the beats of many owners
// (heartbeat/PySwizzle/PySwizzle.py:279-311 per file, one prime per PySwizzle
// instance, :250-251; cxx/shacham_waters_private.cxx:638-702, one prime per
// `init`, :596-624).
//
// The PRF launches need nothing of the prime that is not in the schedules
// already (each PrfParams carries its own R, nb and topmask), except for the
// conversion alpha -> alpha R mod p that hb_batch_prf_kernel does in its accept
// from the kernel arguments.  Here alpha is stored raw by both PRF kernels and
// the segmented conversion pass of the mixed prove (hb_mixed_mont_kernel,
// hb_mixed.hpp) runs over the group's alpha slots, as hb_mont_kernel does for
// hb_cxx_encode_many: converting in the accept from the record would keep the
// record's pointer and 2 NL more values live across the quad engine, which is
// scratch at NL 32 / 64, while the pass costs one launch and
// no scratch.
//
// A MAC workgroup's blocks belong to one file, so the file's record (modulus,
// C, ss, S, tw, first alpha slot) is workgroup-uniform and read through
// hb_table_ref.  The two shapes stay two kernels and two launches of a group:
// hb_emixed_mac_split_kernel for the files with 2 <= S <= T (lane (k, j) takes
// sector j of block k, the first (T / S) S lanes of the fixed T), and
// hb_emixed_mac_lane_kernel for S = 1 or S > T (a lane per block).  One kernel
// with a workgroup-uniform branch was built first and takes the registers of
// the wider shape for both: 256 VGPRs and 1 wave per SIMD at NL 32 where the
// split shape alone has 2, for the shape that PySwizzle's
// defaults take.  The workgroup table holds the split shape's entries first.
//
// Launches per group, both entry points: PRF, conversion, and one MAC launch
// per shape that has a workgroup -- 3 for a group whose files all take one
// shape, 4 for one with both; a cxx group none of whose blocks reads a sector
// has no MAC launch (2).
#pragma once
#include "hb_cbatch.hpp"
#include "hb_mixed.hpp"
#include "hb_emixed_args.hpp"

// F(k) and alpha_j as limbs, as the PRF returned them, at a wave-uniform target
template <int NL>
struct EmPrfHandler {
    u32 *out;       // the file's F values or alpha slots
    __device__ __forceinline__ u64 x_of(u64 job) const { return job; }
    __device__ __forceinline__ void init(u64, u32 sr[4]) const { hb_zero_sr(sr); }
    __device__ __forceinline__ void fail(u64) const {}
    __device__ __forceinline__ void accept(u64 job, const u32 v[NL]) const { hb_store_limbs<NL>(out + job * NL, v); }
};

// hb_batch_prf_kernel with the alpha destination from the file's record
template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_emixed_prf_kernel(EmPrfArgs<NL> A) {
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
        const u64 slot0 = hb_table_ref(A.recs, file).slot0;
        u32 *out = alpha ? A.araw + slot0 * NL : A.fv + F.fbase * NL;
        EmPrfHandler<NL> h{out};
        hb_engine_quad<NL, NR, EmPrfHandler<NL>>(h, L, P, (u64)first + count, A.queue + (alpha ? HB_QSLOT : 0), 16,
                                                  (u64)first);
    }
}

// hb_cbatch_prf_kernel with C, tw and the alpha destination from the file's
// record; the block that reads no sector is decided with the file's own C
template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_cemixed_prf_kernel(CemPrfArgs<NL> A) {
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
        const u64 first = __builtin_amdgcn_readfirstlane(J.first);
        const u64 stop = first + __builtin_amdgcn_readfirstlane(J.count);
        PrfParams<NL> P;
        hb_load_uniform(A.prf, 2u * item + kind, P);
        BatchFile F;
        hb_load_uniform(A.files, item, F);
        const MxRec<NL> &R = hb_table_ref(A.recs, item);
        const u64 C = R.C;
        const u32 tw = R.tw;
        u32 *fv = A.fv + F.fbase * NL, *araw = A.araw + (u64)R.slot0 * NL;
        HbPool pool{first, stop, stop, nullptr, true, 0};
        u64 job = 0;
        bool active = pool.take(__ballot(1), true, job);
        u32 dig[8], sr[4] = {0, 0, 0, 0}, out[NL];
        if (active) hb_sha256_le32((u32)job, dig);
        u32 tries = 0, job_tries = 0;
        while (__ballot(active)) {
            u32 ok = hb_cxx_try<NL, NR>(L, P, sr, dig, out);
            tries += active ? 1u : 0u;
            job_tries += 1u;
            if (job_tries >= HB_CXX_MAX_TRIES) ok = 1;   // `count++ < 80` (prf.hxx:142)
            const bool acc = active && ok;
            if (acc) {
                u32 *dst = (kind == HB_CB_ALPHA ? araw : fv) + job * NL;
                hb_store_limbs<NL>(dst, out);
                if (kind == HB_CB_F && job * C >= F.len) hb_cb_keep_tag(dst, F.tags + job * (u64)tw, tw);
            }
            if constexpr (HB_CB_JOB > 64) {
                const u64 m = __ballot(acc);
                if (m) {
                    u64 nj = 0;
                    const bool got = pool.take(m, acc, nj);
                    if (acc) {
                        active = got;
                        job = nj;
                        job_tries = 0;
                        if (got) {
                            hb_zero_sr(sr);   // resynchronised per evaluate (prf.hxx:132)
                            hb_sha256_le32((u32)job, dig);
                        }
                    }
                }
            } else if (acc) {
                active = false;
            }
        }
        for (int off = 32; off > 0; off >>= 1) tries += __shfl_xor(tries, off);
        if (hb_lane_id() == 0 && tries) atomicAdd(A.queue + kind * HB_QSLOT + 1, (unsigned long long)tries);
    }
}

// hb_batch_mac_split_kernel (2 <= S <= T) with the modulus, C, ss, S, tw and
// the first alpha slot of the workgroup's file.  T threads whatever S is;
// workgroup w takes blocks [first, first + T / S) of file wgs[w].file, lane
// (k, j) sector j of block k; lanes from (T / S) S on only meet the barrier.
// Sector values as everywhere: BE(data[off, min(off + ss, len))), 0 past the
// end of the file.
template <int NL>
__global__ __launch_bounds__(HbMacSplit<NL>::T) void hb_emixed_mac_split_kernel(EmMacArgs<NL> A) {
    constexpr u32 T = HbMacSplit<NL>::T;
    __shared__ u32 red[T * NL];
    BatchMacWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    const u32 file = __builtin_amdgcn_readfirstlane(W.file);
    BatchFile F;
    hb_load_uniform(A.files, file, F);
    const MxRec<NL> &R = hb_table_ref(A.recs, file);
    const u64 C = R.C;
    const u32 ss = R.ss, S = R.S, tw = R.tw, bpw = T / S;
    const u32 lb = threadIdx.x / S, j = threadIdx.x % S;
    const u64 k = (u64)W.first + lb;
    const bool live = lb < bpw && k < F.nblocks;
    const u32 *fv = A.fv + (F.fbase + k) * NL;
    const u32 *am = A.amont + ((u64)R.slot0 + j) * NL;
    if (live) {
        u32 acc[2 * NL + 1], m[NL];
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        if (j == 0)
            for (int t = 0; t < NL; ++t) acc[NL + t] = fv[t];
        const u64 off = k * C + (u64)j * ss;
        if (off < F.len) {
            const u32 r = (u32)(F.len - off < ss ? F.len - off : ss);
            if ((F.flags & HB_BF_LOAD16) && r == ss) hb_load_full16<NL>(F.data, off, m);
            else hb_load_be_bytes<NL>(F.data, off, r, m);
            hb_mac<NL>(acc, am, m);
        }
        u32 v[NL + 1], res[NL];
        hb_redc<NL>(acc, R.mod, v);
        hb_reduce_small<NL>(v, R.mod, res);
        for (int t = 0; t < NL; ++t) red[threadIdx.x * NL + t] = res[t];
    }
    __syncthreads();   // every lane of the workgroup: none has left
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
    hb_reduce_small<NL>(v, R.mod, tag);
    hb_batch_store_tag<NL>(F, k, tw, tag);
}

// hb_batch_mac_kernel (S = 1 or S > T) with the file's record: one lane per
// block, workgroup w takes blocks [first, first + 256) of file wgs[w].file.
template <int NL>
__global__ __launch_bounds__(256) void hb_emixed_mac_lane_kernel(EmMacArgs<NL> A) {
    BatchMacWg W;
    hb_load_uniform(A.wgs, blockIdx.x, W);
    const u32 file = __builtin_amdgcn_readfirstlane(W.file);
    BatchFile F;
    hb_load_uniform(A.files, file, F);
    const u64 k = (u64)W.first + threadIdx.x;
    if (k >= F.nblocks) return;
    const MxRec<NL> &R = hb_table_ref(A.recs, file);
    u32 Fv[NL], tag[NL];
    for (int t = 0; t < NL; ++t) Fv[t] = A.fv[(F.fbase + k) * NL + t];
    const u32 *am = A.amont + (u64)R.slot0 * NL;
    if (F.flags & HB_BF_LOAD16) hb_block_tag<NL, 16>(F.data, F.len, k, R.C, R.ss, R.S, am, R.mod, Fv, tag);
    else hb_block_tag<NL, 1>(F.data, F.len, k, R.C, R.ss, R.S, am, R.mod, Fv, tag);
    hb_batch_store_tag<NL>(F, k, R.tw, tag);
}

template <int NL>
hipError_t hb_launch_emixed_prf(const EmPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_emixed_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_emixed_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_emixed_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_cemixed_prf(const CemPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_cemixed_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_cemixed_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_cemixed_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

// threads per workgroup of the split shape (the host builds the workgroup table
// with hb_em_bpw(T, S), hb_emixed_host.hpp)
template <int NL>
u32 hb_emixed_mac_threads() {
    return HbMacSplit<NL>::T;
}

// A.wgs: the table's first nsplit entries are the split shape's workgroups,
// the nlane entries behind them the lane-per-block shape's; a launch each,
// none for a shape without workgroups.
template <int NL>
hipError_t hb_launch_emixed_mac(const EmMacArgs<NL> &A, u32 nsplit, u32 nlane, hipStream_t s) {
    if (nsplit) HB_LAUNCH((hb_emixed_mac_split_kernel<NL>), dim3(nsplit), dim3(HbMacSplit<NL>::T), s, A);
    if (nlane) {
        EmMacArgs<NL> B = A;
        B.wgs = A.wgs + nsplit;
        HB_LAUNCH((hb_emixed_mac_lane_kernel<NL>), dim3(nlane), dim3(256), s, B);
    }
    return hipGetLastError();
}

#define HB_INST_EMIXED(NL)                                                                          \
    template hipError_t hb_launch_emixed_prf<NL>(const EmPrfArgs<NL> &, int, int, hipStream_t);    \
    template hipError_t hb_launch_cemixed_prf<NL>(const CemPrfArgs<NL> &, int, int, hipStream_t);  \
    template u32 hb_emixed_mac_threads<NL>();                                                       \
    template hipError_t hb_launch_emixed_mac<NL>(const EmMacArgs<NL> &, u32, u32, hipStream_t);
