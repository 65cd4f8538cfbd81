// The Merkle scheme's kernels (heartbeat/Merkle/Merkle.py:323-367 encode,
// :388-404 prove): the seed chains, the leaves (chunk position, chunk HMAC,
// leaf hash) and the trees of a batch of files, three launches in all.
#include "hb_kernels.hpp"
#include "hb_merkle_args.hpp"

// ------------------------------------------------------------------ seed chains
// A lane per file: s_1 is the host's (a generic HMAC of the caller's seed),
// s_{k+1} = HMAC(key, s_k) on the file's key midstates, two compressions a link.
__global__ __launch_bounds__(64) void hb_merkle_chain_kernel(MkChainArgs A) {
    const u64 f = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.nfiles) return;
    const MkFile &F = A.files[f];
    const HbMkKey K = F.key;
    u32 s[8];
    for (int t = 0; t < 8; ++t) s[t] = F.s1[t];
    u32 *out = A.seeds + F.job0 * 8;
    HB_NOUNROLL
    for (u32 k = 0; k < F.n; ++k) {
        for (int t = 0; t < 8; ++t) out[(u64)k * 8 + t] = hb_bswap(s[t]);
        if (k + 1 < F.n) {
            u32 nx[8];
            hb_mk_link(K, s, nx);
            for (int t = 0; t < 8; ++t) s[t] = nx[t];
        }
    }
}

// ------------------------------------------------------------------ leaves
// The file of a flat job: the last f with files[f].job0 <= job.
__device__ __forceinline__ u64 hb_mk_file_of(const MkFile *files, u64 nfiles, u64 job) {
    u64 lo = 0, hi = nfiles;   // files[lo].job0 <= job < files[hi].job0 (hi = nfiles: the end)
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (files[mid].job0 <= job) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A lane per (file, leaf): the seed's AES schedule, the chunk position
// KeyedPRF(seed, filesz - chunk + 1).eval(0) under the file's own range, the
// chunk's HMAC under the seed (the leaf blob) and the leaf hash into node
// 2^order - 1 + leaf of the file.  Lanes of a wave may belong to files of
// different chunk lengths: every loop bound below is the lane's own.
template <int NR>
__global__ __launch_bounds__(256) void hb_merkle_leaves_kernel(MkLeavesArgs A) {
    __shared__ __attribute__((aligned(16))) u32 lds[HB_LDS_WORDS];
    hb_fill_lds(lds, A.t0);
    const LaneTab L = hb_lane_tab(lds);
    const u64 job = A.job_lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (job >= A.job_hi) return;
    const MkFile &F = A.files[hb_mk_file_of(A.files, A.nfiles, job)];
    const u32 gather = F.flags & HB_MK_GATHER;
    if (A.pass == 1 && !gather) return;
    const u64 leaf = job - F.job0;
    const u32 *sd = A.seeds + job * 8;
    constexpr int NK = NR - 6;
    u64 pos;
    if (A.pass == 0) {
        u32 key[NK];
        for (int t = 0; t < NK; ++t) key[t] = sd[t];   // AES key words are little-endian
        PrfParams<2> P;
        hb_aes_expand_lane<NR>(L, key, P.rk);
        P.R[0] = F.R[0];
        P.R[1] = F.R[1];
        P.nb = F.nb;
        P.topmask = F.topmask;
        u32 sr[4] = {0, 0, 0, 0}, out[2] = {0, 0}, ok = 0;
        for (u32 t = 0; t < HB_MAX_TRIES && !ok; ++t) ok = hb_prf_try<2, NR>(L, P, sr, A.dig0, out);
        if (!ok) {
            atomicOr(A.flags, 2u);
            return;
        }
        pos = (u64)out[0] | ((u64)out[1] << 32);
        A.offsets[job] = pos;
        if (gather) return;
    } else {
        pos = leaf * F.chunk;   // the gathered chunks, in leaf order
    }
    // nothing is read outside [data, data + len), whatever the table says
    if (pos > F.len || F.len - pos < F.chunk) {
        atomicOr(A.flags, 4u);
        return;
    }
    u32 kw[16];
    for (int t = 0; t < 16; ++t) kw[t] = t < NK ? hb_bswap(sd[t]) : 0u;
    u32 d[8];
    hb_hmac_sha256(kw, F.data, F.len, pos, F.chunk, d);
    for (int t = 0; t < 8; ++t) A.blobs[job * 8 + t] = hb_bswap(d[t]);
    if (A.nodes) {
        u32 h[8];
        hb_mk_leaf_hash(d, (u32)leaf, h);
        u32 *nd = A.nodes + (F.node0 + ((u64)1 << F.order) - 1 + leaf) * 8;
        for (int t = 0; t < 8; ++t) nd[t] = hb_bswap(h[t]);
    }
}

// ------------------------------------------------------------------ trees
// A workgroup per file: level by level from the leaves' parents to the root,
// lanes strided over a level's nodes.  The nodes live in the output buffer.
__global__ __launch_bounds__(256) void hb_merkle_tree_kernel(MkTreeArgs A) {
    const MkFile &F = A.files[blockIdx.x];
    const u32 order = F.order, n = F.n;
    u32 *nodes = A.nodes + F.node0 * 8;
    for (u32 i = 1; i <= order; ++i) {
        const u32 p = 1u << (order - i);
        for (u32 j = threadIdx.x; j < p; j += blockDim.x) hb_mk_tree_node(nodes, order, n, i, j);
        __syncthreads();
    }
}

hipError_t hb_launch_merkle_chain(const MkChainArgs &A, hipStream_t s) {
    const u64 grid = (A.nfiles + 63) / 64;
    hipLaunchKernelGGL(hb_merkle_chain_kernel, dim3((u32)grid), dim3(64), 0, s, A);
    return hipGetLastError();
}

hipError_t hb_launch_merkle_leaves(const MkLeavesArgs &A, int nr, hipStream_t s) {
    const u64 grid = (A.job_hi - A.job_lo + 255) / 256;
    dim3 g((u32)grid), b(256);
    if (nr == 14) hipLaunchKernelGGL((hb_merkle_leaves_kernel<14>), g, b, 0, s, A);
    else if (nr == 12) hipLaunchKernelGGL((hb_merkle_leaves_kernel<12>), g, b, 0, s, A);
    else hipLaunchKernelGGL((hb_merkle_leaves_kernel<10>), g, b, 0, s, A);
    return hipGetLastError();
}

hipError_t hb_launch_merkle_tree(const MkTreeArgs &A, u64 nfiles, hipStream_t s) {
    hipLaunchKernelGGL(hb_merkle_tree_kernel, dim3((u32)nfiles), dim3(256), 0, s, A);
    return hipGetLastError();
}
