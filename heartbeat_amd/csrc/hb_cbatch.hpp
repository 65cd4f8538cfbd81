// hb_cbatch.hpp -- the PRF launch of the batched cxx encode (hb_cxx_encode_many;
// instantiated by hb_kern_cbatch.hip and hb_kern_cbatch64.hip): F(k) of every
// block and alpha_j of every sector of many small files, each under its own
// f_key and alpha_key, with the cxx prf (cxx/prf.hxx:125-176).  Replaces an
// uploader's loop over cxx/shacham_waters_private.cxx:638-702 (one hb_encode
// with HB_PRF_CXX per file: a single-pass engine launch and an alpha launch
// each).
//
// The queue, the tables and the scalar loads are the other batch PRF kernels'
// (hb_batch.hpp).  The engine is not: a try of the cxx prf is nb / 16 full AES
// blocks (8 at 1024 bits) where a KeyedPRF try is nb serial CFB-8 steps, so
// there is no long chain for the four lanes of a quad to share
// (hb_engine_quad is KeyedPRF only).  One lane runs one evaluation, and a
// wave-job is up to HB_CB_JOB evaluations of one item under one key.  The
// per-lane functions are the single calls' (hb_sha256_le32, hb_cxx_try), so
// the 81-try rule has one place.
#pragma once
#include "hb_batch.hpp"
#include "hb_cbatch_args.hpp"

// The tag of a block that reads no sector (hb_cbatch_args.hpp: at most the last
// block of a file) is F as the PRF returned it: the tw low bytes of the limbs
// the lane has just stored at `limbs`, big-endian.  A rolled loop over memory
// on purpose: the unrolled byte stores of hb_store_be_bytes in the accept kept
// 4 NL more values live (116 / 556 / 1,476 B of scratch per lane at NL 8 / 16 /
// 32 against none), for a store that one lane per file runs.
__device__ __forceinline__ void hb_cb_keep_tag(const u32 *limbs, unsigned char *dst, u32 tw) {
    HB_NOUNROLL
    for (u32 pos = 0; pos < tw; ++pos) dst[tw - 1 - pos] = (unsigned char)(limbs[pos >> 2] >> (8 * (pos & 3u)));
}

template <int NL, int NR>
__global__ __launch_bounds__(HB_ENGINE_WG) void hb_cbatch_prf_kernel(CbPrfArgs<NL> A) {
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
        u32 *fv = A.fv + F.fbase * NL, *araw = A.araw + (u64)item * A.S * NL;
        // evaluations [first, stop) dealt from a wave-local pool that never
        // refills: queue[0] is the wave-jobs' counter, not the engine's.  With
        // HB_CB_JOB = 64 the first deal empties it.
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
                if (kind == HB_CB_F && job * A.C >= F.len) hb_cb_keep_tag(dst, F.tags + job * (u64)A.tw, A.tw);
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

template <int NL>
hipError_t hb_launch_cbatch_prf(const CbPrfArgs<NL> &A, int nr, int grid, hipStream_t s) {
    dim3 g(grid), b(HB_ENGINE_WG);
    if (nr == 14) HB_LAUNCH((hb_cbatch_prf_kernel<NL, 14>), g, b, s, A);
    else if (nr == 12) HB_LAUNCH((hb_cbatch_prf_kernel<NL, 12>), g, b, s, A);
    else HB_LAUNCH((hb_cbatch_prf_kernel<NL, 10>), g, b, s, A);
    return hipGetLastError();
}

#define HB_INST_CBATCH(NL) \
    template hipError_t hb_launch_cbatch_prf<NL>(const CbPrfArgs<NL> &, int, int, hipStream_t);
