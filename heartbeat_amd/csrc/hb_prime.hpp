// hb_prime.hpp -- drawing primes on the GPU (hb_mr_test, hb_prime_search):
// the per-lane strong-probable-prime test and the sieve's per-prime step, and
// (device builds only) the two kernels over them, instantiated by
// hb_kern_prime.hip, hb_kern_prime32.hip and hb_kern_prime64.hip.
//
// Replaces the host loop of getPrime (heartbeat/PySwizzle/PySwizzle.py:74-77,
// heartbeat/util.py): trial division, then Miller-Rabin rounds of pow().
//
// The lane code compiles as HIP device code and as plain C++ (tests/primeemul)
// like hb_lane.hpp, whose hb_mac / hb_redc / hb_madc it uses.  Every lane has
// its own modulus, so every Montgomery constant is derived in the lane:
//   * -n^-1 mod 2^32 by Newton steps;
//   * R mod n (R = 2^(32 NL)) by modular doublings from 2^(bitlen(n) - 1) < n;
//   * R^2 mod n by 32 NL further doublings;
//   * a R as one Montgomery product with R^2.
// After a REDC the value is < 2n; one conditional subtraction keeps residues
// canonical (< n), so x == 1 is x == R mod n and x == -1 is x + R mod n == n.
// ModP's inv_scaled and hb_reduce_small are not used.
#pragma once
#if defined(__HIPCC__)
#include "hb_kernels.hpp"   // hip_runtime.h, hb_lane.hpp, HB_LAUNCH, hb_load_kernel
#else
#include "hb_lane.hpp"
#endif

// bit length of x (NL limbs), 0 for x == 0
template <int NL>
HB_HD u32 hb_pr_bitlen(const u32 x[NL]) {
    u32 L = 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t)
        if (x[t]) L = 32u * (u32)t + 32u - (u32)__builtin_clz(x[t]);
    return L;
}

// x = 2x mod n for x < n
template <int NL>
HB_HD void hb_pr_double(u32 x[NL], const u32 n[NL]) {
    u32 y[NL], d[NL];
    u32 carry = 0, borrow = 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) {
        y[t] = (x[t] << 1) | carry;
        carry = x[t] >> 31;
        const u64 s = (u64)y[t] - n[t] - borrow;
        d[t] = (u32)s;
        borrow = (u32)(s >> 63);
    }
    const bool sub = carry != 0 || borrow == 0;   // 2x >= n
    HB_UNROLL
    for (int t = 0; t < NL; ++t) x[t] = sub ? d[t] : y[t];
}

// hb_mac for limb counts that do not fit the register file: the same product
// scanning with rolled loops, the operands in scratch.
template <int NL>
HB_HD void hb_pr_mac_rolled(u32 *acc, const u32 *a, const u32 *b) {
    u64 lo = 0;
    u32 hi = 0;
    for (int t = 0; t < 2 * NL - 1; ++t) {
        const int a0 = t < NL ? 0 : t - NL + 1, a1 = t < NL ? t : NL - 1;
        for (int i = a0; i <= a1; ++i) hb_madc(lo, hi, a[i], b[t - i]);
        acc[t] = (u32)lo;
        lo = (lo >> 32) | ((u64)hi << 32);
        hi = 0;
    }
    acc[2 * NL - 1] = (u32)lo;
    acc[2 * NL] = 0;
}

// x = x * b / R mod n, canonical (x, b < n; M.p = n, M.pinv set)
template <int NL>
HB_HD void hb_pr_mul(u32 x[NL], const u32 b[NL], const ModP<NL> &M) {
    u32 acc[2 * NL + 1], v[NL + 1], d[NL];
    if constexpr (NL <= 32) {
        HB_UNROLL
        for (int t = 0; t <= 2 * NL; ++t) acc[t] = 0;
        hb_mac<NL>(acc, x, b);
    } else {
        hb_pr_mac_rolled<NL>(acc, x, b);
    }
    hb_redc<NL>(acc, M, v);   // v < 2n
    u32 borrow = 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) {
        const u64 s = (u64)v[t] - M.p[t] - borrow;
        d[t] = (u32)s;
        borrow = (u32)(s >> 63);
    }
    const bool sub = v[NL] != 0 || borrow == 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) x[t] = sub ? d[t] : v[t];
}

template <int NL>
HB_HD bool hb_pr_equal(const u32 a[NL], const u32 b[NL]) {
    u32 diff = 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) diff |= a[t] ^ b[t];
    return diff == 0;
}

// a + b == n  (a, b < n): x == -1 for b = R mod n
template <int NL>
HB_HD bool hb_pr_sum_is(const u32 a[NL], const u32 b[NL], const u32 n[NL]) {
    u32 diff = 0, carry = 0;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) {
        const u64 s = (u64)a[t] + b[t] + carry;
        carry = (u32)(s >> 32);
        diff |= (u32)s ^ n[t];
    }
    return (diff | carry) == 0;
}

// Is odd n >= 5 (NL little-endian limbs) a strong probable prime to base a,
// 2 <= a <= n - 2?  base2: a is 2 and need not be read; the multiply of the
// exponentiation is then a modular doubling.  maxbits >= bitlen(n) bounds the
// scan (the call's largest candidate; the same for every lane of a launch).
//
// One uniform scan over bits maxbits-1 .. 0 of n - 1 = d 2^s: square, then
// multiply by (bit ? a R : 1 R) -- always, so the lanes of a wave stay
// together whatever their bits.  Bits above bitlen(n) keep x = 1; the bits of
// d are the ladder; at bit s (x = a^d) accept on x in {1, -1}; on bits
// s-1 .. 1 the multiply is by 1 and the squares give a^(d 2^r), r < s: accept
// on -1.  s is lane state, never a trip count.
template <int NL>
HB_HD bool hb_sprp_lane(const u32 n[NL], const u32 a[NL], bool base2, u32 maxbits = 32u * NL) {
    ModP<NL> M;
    {
        u32 inv = 1;
        HB_UNROLL
        for (int i = 0; i < 5; ++i) inv *= 2u - n[0] * inv;
        M.pinv = 0u - inv;
    }
    u32 s = 0;   // trailing zero bits of n - 1
    {
        bool seen = false;
        HB_UNROLL
        for (int t = 0; t < NL; ++t) {
            M.p[t] = n[t];
            const u32 w = t == 0 ? n[0] & ~1u : n[t];
            if (!seen && w) {
                s = 32u * (u32)t + (u32)__builtin_ctz(w);
                seen = true;
            }
        }
    }
    const u32 L = hb_pr_bitlen<NL>(n);
    // one = R mod n: 2^(L-1), doubled 32 NL - (L - 1) times
    u32 one[NL];
    HB_UNROLL
    for (int t = 0; t < NL; ++t) one[t] = (u32)t == (L - 1) / 32 ? 1u << ((L - 1) % 32) : 0u;
    HB_NOUNROLL
    for (u32 i = 0; i < 32u * NL; ++i) {
        if (i + 1 < L) continue;
        hb_pr_double<NL>(one, M.p);
    }
    u32 ar[NL];   // a R mod n (unused for base 2)
    if (!base2) {
        u32 r2[NL];
        HB_UNROLL
        for (int t = 0; t < NL; ++t) r2[t] = one[t];
        HB_NOUNROLL
        for (u32 i = 0; i < 32u * NL; ++i) hb_pr_double<NL>(r2, M.p);
        HB_UNROLL
        for (int t = 0; t < NL; ++t) ar[t] = a[t];
        hb_pr_mul<NL>(ar, r2, M);
    }
    // e: n - 1 shifted so that bit maxbits-1 is the top bit of the top limb
    u32 e[NL], x[NL];
    HB_UNROLL
    for (int t = 0; t < NL; ++t) {
        e[t] = t == 0 ? n[0] & ~1u : n[t];
        x[t] = one[t];
    }
    HB_NOUNROLL
    for (u32 i = maxbits; i < 32u * NL; ++i) {
        HB_UNROLL
        for (int t = NL - 1; t > 0; --t) e[t] = (e[t] << 1) | (e[t - 1] >> 31);
        e[0] <<= 1;
    }
    bool ok = false;
    HB_NOUNROLL
    for (u32 i = maxbits; i-- > 0;) {
        const bool bit = (e[NL - 1] >> 31) != 0;
        HB_UNROLL
        for (int t = NL - 1; t > 0; --t) e[t] = (e[t] << 1) | (e[t - 1] >> 31);
        e[0] <<= 1;
        if (base2) {
            hb_pr_mul<NL>(x, x, M);
            u32 y[NL];
            HB_UNROLL
            for (int t = 0; t < NL; ++t) y[t] = x[t];
            hb_pr_double<NL>(y, M.p);
            HB_UNROLL
            for (int t = 0; t < NL; ++t) x[t] = bit ? y[t] : x[t];
        } else {
            // one Montgomery product in the loop body, run twice: x * x, then
            // x * (a R or 1 R)
            HB_NOUNROLL
            for (int h = 0; h < 2; ++h) {
                u32 b[NL];
                HB_UNROLL
                for (int t = 0; t < NL; ++t) b[t] = h == 0 ? x[t] : bit ? ar[t] : one[t];
                hb_pr_mul<NL>(x, b, M);
            }
        }
        const bool minus = hb_pr_sum_is<NL>(x, one, M.p);
        const bool plus = hb_pr_equal<NL>(x, one);
        ok = ok || (i == s && (plus || minus)) || (i < s && i >= 1 && minus);
    }
    return ok;
}

// ------------------------------------------------------------------ sieve
// The smallest k >= 0 with start + 2k == 0 (mod q), q an odd prime < 2^16:
// r = start mod q by Horner over 16-bit halves, k = (q - r) / 2 mod q.
template <int NL>
HB_HD u32 hb_sieve_first_k(const u32 *start, u32 q) {
    u32 r = 0;
    for (int t = NL - 1; t >= 0; --t) {
        r = ((r << 16) | (start[t] >> 16)) % q;
        r = ((r << 16) | (start[t] & 0xffffu)) % q;
    }
    const u32 m = r ? q - r : 0u;        // -start mod q
    return (m * ((q + 1u) >> 1)) % q;    // < 2^31: q < 2^16
}

// start + 2k as NL limbs (the caller keeps it below 2^(32 NL))
template <int NL>
HB_HD void hb_pr_candidate(const u32 *start, u32 k, u32 n[NL]) {
    u64 c = 2ull * k;
    HB_UNROLL
    for (int t = 0; t < NL; ++t) {
        c += start[t];
        n[t] = (u32)c;
        c >>= 32;
    }
}

#if defined(__HIPCC__)
#include "hb_prime_args.hpp"

// ------------------------------------------------------------------ kernels
// One lane per job (candidate, base).  A workgroup is one wave, so that a few
// thousand lanes already spread over every CU and the compiler may give a lane
// the whole register file (512 VGPRs at one wave per SIMD).
template <int NL, bool BASE2>
__global__ __launch_bounds__(HB_PR_TEST_WG) void hb_prime_test_kernel(PrTestArgs A) {
    const u64 j = (u64)blockIdx.x * HB_PR_TEST_WG + threadIdx.x;
    if (j >= A.njobs) return;
    const PrJob J = A.jobs[j];
    u32 n[NL], a[NL];
    hb_pr_candidate<NL>(A.src + (u64)J.src * NL, J.k, n);
    if constexpr (!BASE2) {
        const u32 *b = A.bases + (u64)J.base * NL;
        for (int t = 0; t < NL; ++t) a[t] = b[t];
    } else {
        for (int t = 0; t < NL; ++t) a[t] = 0;
    }
    A.pass[j] = hb_sprp_lane<NL>(n, a, BASE2, A.maxbits) ? 1u : 0u;
}

// One workgroup per start: flag[k] (LDS, a byte per odd candidate start + 2k,
// k < win[start]) is cleared for every k with a sieve prime q | start + 2k
// other than q itself; the survivors' k go to surv[start * stride ..] in
// ascending order, their number to count[start].  Byte stores of 0 from
// several threads to one flag are the only races.
template <int NL>
__global__ __launch_bounds__(HB_PR_SIEVE_WG) void hb_prime_sieve_kernel(PrSieveArgs A) {
    constexpr u32 WORDS = HB_PR_MAX_WINDOW / 32u, PER = WORDS / HB_PR_SIEVE_WG;
    __shared__ u32 map[WORDS];
    __shared__ u32 part[HB_PR_SIEVE_WG];
    const u32 tid = threadIdx.x;
    const u32 *start = A.starts + (u64)blockIdx.x * NL;
    const u32 win = A.win[blockIdx.x] < HB_PR_MAX_WINDOW ? A.win[blockIdx.x] : HB_PR_MAX_WINDOW;
    for (u32 w = tid; w < WORDS; w += HB_PR_SIEVE_WG)
        map[w] = 32u * w + 32u <= win ? 0xffffffffu : 32u * w < win ? (1u << (win - 32u * w)) - 1u : 0u;
    __syncthreads();
    // start itself can be a sieve prime only below 2^16
    bool small = start[0] < 65536u;
    for (int t = 1; t < NL; ++t) small = small && start[t] == 0;
    for (u32 i = tid; i < A.nq; i += HB_PR_SIEVE_WG) {
        const u32 q = A.q[i];
        for (u32 k = hb_sieve_first_k<NL>(start, q); k < win; k += q)
            if (!(small && start[0] + 2u * k == q)) atomicAnd(&map[k >> 5], ~(1u << (k & 31u)));
    }
    __syncthreads();
    // thread t compacts words [t * PER, (t + 1) * PER)
    u32 mine = 0;
    for (u32 w = 0; w < PER; ++w) mine += (u32)__builtin_popcount(map[tid * PER + w]);
    part[tid] = mine;
    __syncthreads();
    for (u32 d = 1; d < HB_PR_SIEVE_WG; d <<= 1) {
        const u32 v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u32 pos = part[tid] - mine;
    unsigned short *out = A.surv + (u64)blockIdx.x * A.stride;
    for (u32 w = 0; w < PER; ++w) {
        const u32 m = map[tid * PER + w];
        for (u32 b = 0; b < 32u; ++b)
            if ((m >> b) & 1u) out[pos++] = (unsigned short)(32u * (tid * PER + w) + b);
    }
    if (tid == HB_PR_SIEVE_WG - 1) A.count[blockIdx.x] = part[tid];
}

template <int NL>
hipError_t hb_launch_prime_test(const PrTestArgs &A, bool base2, hipStream_t s) {
    const dim3 g((unsigned)((A.njobs + HB_PR_TEST_WG - 1) / HB_PR_TEST_WG)), b(HB_PR_TEST_WG);
    if (base2) HB_LAUNCH((hb_prime_test_kernel<NL, true>), g, b, s, A);
    else HB_LAUNCH((hb_prime_test_kernel<NL, false>), g, b, s, A);
    return hipGetLastError();
}

template <int NL>
hipError_t hb_launch_prime_sieve(const PrSieveArgs &A, u32 nstarts, u32 window, hipStream_t s) {
    const dim3 g(nstarts), b(HB_PR_SIEVE_WG);
    const u32 lds = (window + 3u) & ~3u;
    if (hb_load_only) hb_load_kernel(&hb_prime_sieve_kernel<NL>);
    else if (!nstarts) return hipErrorInvalidConfiguration;
    else hipLaunchKernelGGL((hb_prime_sieve_kernel<NL>), g, b, lds, s, A);
    return hipGetLastError();
}

#define HB_INST_PRIME(NL)                                                                   \
    template hipError_t hb_launch_prime_test<NL>(const PrTestArgs &, bool, hipStream_t);   \
    template hipError_t hb_launch_prime_sieve<NL>(const PrSieveArgs &, u32, u32, hipStream_t);
#endif
