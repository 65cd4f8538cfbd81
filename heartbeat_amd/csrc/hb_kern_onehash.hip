// The OneHash scheme's kernels (heartbeat/OneHash/OneHash.py:141-168 the seed
// chain, :112-138 the responses): the chains of a batch of files and the
// responses of a batch of jobs, two launches in all.
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
