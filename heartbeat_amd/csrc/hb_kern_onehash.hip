// The OneHash scheme's kernels (heartbeat/OneHash/OneHash.py:141-168 the seed
// chain, :112-138 the responses, :170-189 the positions): the chains of a
// batch of files and the responses of a batch of jobs, two launches in all,
// and the positions of a batch of files, a third.
#include "hb_kernels.hpp"
#include "hb_onehash_args.hpp"

// ------------------------------------------------------------------ seed chains
// A lane per file: s_0 is the host's (SHA-256 of the root seed),
// s_{k+1} = SHA-256(s_k || secret) on the file's prepared secret, one or two
// compressions a link.
__global__ __launch_bounds__(64) void hb_onehash_chain_kernel(OhChainArgs A) {
    const u64 f = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.nfiles) return;
    const OhFile &F = A.files[f];
    if (F.flags & HB_OH_HOST_CHAIN) return;
    const HbOhSecret S = F.secret;
    u32 s[8];
    for (int t = 0; t < 8; ++t) s[t] = F.s0[t];
    u32 *out = A.seeds + F.job0 * 8;
    HB_NOUNROLL
    for (u32 k = 0; k < F.n; ++k) {
        for (int t = 0; t < 8; ++t) out[(u64)k * 8 + t] = hb_bswap(s[t]);
        if (k + 1 < F.n) {
            u32 nx[8];
            hb_oh_link(S, s, nx);
            for (int t = 0; t < 8; ++t) s[t] = nx[t];
        }
    }
}

// ------------------------------------------------------------------ responses
// The file of a flat job: the last f with files[f].job0 <= job.
__device__ __forceinline__ u64 hb_oh_file_of(const OhFile *files, u64 nfiles, u64 job) {
    u64 lo = 0, hi = nfiles;   // files[lo].job0 <= job < files[hi].job0 (hi = nfiles: the end)
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (files[mid].job0 <= job) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A lane per job = (file, block, seed): the plan rule, the segments' bounds,
// the hash, 32 bytes out.  Lanes of a wave may belong to files of different
// sizes and chunk lengths, and their seeds may differ in length: every loop
// bound is the lane's own.  No LDS; a workgroup is one wave, so that a batch
// of a few thousand jobs still reaches every compute unit.
__global__ __launch_bounds__(64) void hb_onehash_resp_kernel(OhRespArgs A) {
    const u64 job = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= A.njobs) return;
    const OhFile &F = A.files[hb_oh_file_of(A.files, A.nfiles, job)];
    const u64 block = *(const u64 *)(A.blocks + job * A.block_stride);
    const u64 seed_len = A.seed_lens ? *(const u64 *)(A.seed_lens + job * A.len_stride) : 32;
    const u64 fsz = F.file_size;
    // nothing is read outside [data, data + len), whatever the tables say
    bool ok = seed_len <= HB_ONEHASH_MAX_SEED && (block < fsz || (block == 0 && fsz == 0));
    HbOhPlan P = {0, 0, 0, 0};
    if (ok) {
        P = hb_oh_plan(fsz, block);
        if (F.flags & HB_OH_GATHER) {
            P.off0 = (job - F.job0) * hb_oh_chunk(fsz);
            P.off1 = P.off0 + P.len0;
        }
        ok = hb_oh_plan_inside(P, F.len);
    }
    if (!ok) {
        atomicOr(A.flags, 4u);
        return;
    }
    u32 d[8];
    hb_oh_hash(F.data, F.len, P, A.seeds + job * A.seed_stride, seed_len, d);
    for (int t = 0; t < 8; ++t) A.resp[job * 8 + t] = hb_bswap(d[t]);
}

// ------------------------------------------------------------------ positions
// A wave per file draws the file's positions (pick_blocks, hb_onehash_draw.hpp)
// from one generator state in LDS (2,496 bytes).  Lane 0 seeds it -- a serial
// recurrence.  Then, array by array: the 624 elements are regenerated 64 at a
// time in index order, every chunk reading before it writes; the array's
// attempts are tempered and tested 64 at a time, and the accepted values go
// out in stream order by a ballot and a prefix count, up to the attempt that
// yields the num-th.  The state that comes back is the array in use and the
// words consumed in it: nothing is regenerated past the last attempt.
// A workgroup is one wave, as for the responses: few files, latency-bound.
__global__ __launch_bounds__(64) void hb_onehash_draw_kernel(OhDrawArgs A) {
    __shared__ u32 mt[HB_MT_N];
    const u64 f = blockIdx.x;
    const u32 lane = threadIdx.x;
    if (f >= A.nfiles) return;
    const OhDraw D = A.draws[f];
    if (lane == 0) hb_mt_seed(mt, A.keys + D.key0, D.key_words);
    __syncthreads();
    const u64 num = D.len ? D.num : 0;   // the host has refused len = 0 with num > 0: no attempt could be accepted
    const u32 k = hb_mt_bits(D.len), w = hb_mt_words(k);
    const u32 attempts = HB_MT_N / w;
    u64 *out = A.blocks + D.job0;
    u32 used = HB_MT_N;
    u64 made = 0;
    HB_NOUNROLL
    while (made < num) {
        HB_NOUNROLL
        for (u32 base = 0; base < HB_MT_N; base += HB_MT_CHUNK) {
            const u32 i = base + lane;
            u32 v = 0;
            if (i < HB_MT_N) v = hb_mt_next(mt, i);
            __syncthreads();
            if (i < HB_MT_N) mt[i] = v;
            __syncthreads();
        }
        HB_NOUNROLL
        for (u32 a0 = 0; a0 < attempts; a0 += HB_MT_CHUNK) {
            const u32 a = a0 + lane;
            u64 r = 0;
            const bool ok = a < attempts && hb_mt_attempt(mt, a, D.len, k, r);
            const u64 mask = __ballot(ok);
            const u64 need = num - made;
            const u32 before = (u32)__popcll(mask & ((1ull << lane) - 1ull));
            const u32 total = (u32)__popcll(mask);
            if (ok && before < need) out[made + before] = r;
            if (total >= need) {
                // the lane whose attempt yields the last value closes the stream
                const u64 last = __ballot(ok && before + 1 == need);
                used = (a0 + (u32)__ffsll((unsigned long long)last)) * w;
                made = num;
                break;
            }
            made += total;
            used = (a0 + HB_MT_CHUNK < attempts ? a0 + HB_MT_CHUNK : attempts) * w;
        }
    }
    if (A.states) {
        __syncthreads();
        u32 *st = A.states + f * HB_MT_STATE_WORDS;
        for (u32 i = lane; i < HB_MT_N; i += HB_MT_CHUNK) st[i] = mt[i];
        if (lane == 0) st[HB_MT_N] = used;
    }
}

hipError_t hb_launch_onehash_draw(const OhDrawArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(hb_onehash_draw_kernel, dim3((u32)A.nfiles), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t hb_launch_onehash_chain(const OhChainArgs &A, hipStream_t s) {
    const u64 grid = (A.nfiles + 63) / 64;
    hipLaunchKernelGGL(hb_onehash_chain_kernel, dim3((u32)grid), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t hb_launch_onehash_resp(const OhRespArgs &A, hipStream_t s) {
    const u64 grid = (A.njobs + 63) / 64;
    hipLaunchKernelGGL(hb_onehash_resp_kernel, dim3((u32)grid), dim3(64), 0, s, A);
    return hipGetLastError();
}
