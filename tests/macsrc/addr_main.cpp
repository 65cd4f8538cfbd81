// Sweeps the load addresses of the matrix-core MACs
// (heartbeat_amd/csrc/hb_mac_src.hpp) over file lengths, sector counts, every
// lane of the last two waves and every K slice: each 16-byte read must lie
// wholly inside the file or inside the fallback buffer, and exactly the lanes
// whose block is whole read the file.  The reads are made (memcpy) on heap
// buffers of exactly those sizes; built with -fsanitize=address,undefined and
// run by tests/test_mac_src.py.  Exit status 0 and "ok <n>" on success.
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hb_mac_src.hpp"

static long long g_checks = 0, g_bad = 0;
static unsigned g_sink = 0;

struct Buf {
    unsigned char *p;
    u64 n;
    explicit Buf(u64 bytes) : p((unsigned char *)malloc(bytes ? bytes : 1)), n(bytes) {
        if (!p) abort();
        memset(p, 0x5a, bytes ? bytes : 1);
    }
    ~Buf() { free(p); }
    bool holds(const unsigned char *a) const { return a >= p && (u64)(a - p) + 16 <= n; }
};

static void fail(const char *what, u64 len, u32 S, u32 wave, u32 l, u32 g, u32 step) {
    if (++g_bad <= 20)
        printf("FAIL %s: len %llu S %u wave %u lane %u load %u step %u\n", what, (unsigned long long)len, S, wave, l, g,
               step);
}

// one 16-byte read at a + step: in the file exactly when `ok`, else in the fallback
static void read16(const char *what, const unsigned char *a, u32 step, bool ok, const unsigned char *want,
                   const Buf &file, const Buf &fb, u64 len, u32 S, u32 wave, u32 l, u32 g) {
    ++g_checks;
    const unsigned char *p = a + step;
    const bool in_file = file.holds(p), in_fb = fb.holds(p);
    if (ok ? !(in_file && p == want) : !in_fb) {
        fail(what, len, S, wave, l, g, step);
        return;
    }
    unsigned char v[16];
    memcpy(v, p, 16);
    g_sink += v[0] + v[15];
}

// the 256-bit MACs: C = 32 S, blocks dealt 64 to a wave, job = 64 wave + lane,
// an idle lane holds job 0 (HbPool::take)
static void sweep256(u64 len, u32 S) {
    const u64 C = 32ull * S;
    const u64 nblocks = len / C + 1;   // the callers' count: the short last block included
    const Buf file(len), fb(hb_mac_fallback_bytes(S, 1));
    const u64 nwaves = (nblocks + 63) / 64;
    for (u64 wave = nwaves >= 2 ? nwaves - 2 : 0; wave < nwaves; ++wave) {
        u64 job[64];
        bool act[64], full[64];
        for (u32 l = 0; l < 64; ++l) {
            const u64 j = 64 * wave + l;
            act[l] = j < nblocks;
            job[l] = act[l] ? j : 0;
            full[l] = act[l] && job[l] * C + C <= len;   // the test's own rule
            ++g_checks;
            if (hb_mac_block_ok(act[l], job[l], C, len) != full[l]) fail("block_ok", len, S, (u32)wave, l, 0, 0);
        }
        for (u32 l = 0; l < 64; ++l) {
            if (S % 2 == 0)   // 16x16x64: K slices of 64 bytes
                for (u32 g = 0; g < 4; ++g) {
                    const u32 s = hb_mac16_src_lane(l, g), lo = hb_mac16_lane_off(l);
                    const bool ok = hb_mac_block_ok(act[s], job[s], C, len);
                    const unsigned char *a = hb_mac_src(ok, file.p, job[s], C, fb.p, lo);
                    for (u32 p = 0; p < S / 2; ++p)
                        read16("mac16", a, 64 * p, full[s], file.p + job[s] * C + lo + 64 * p, file, fb, len, S,
                               (u32)wave, l, g);
                }
            if (S % 4 == 0)   // 32x32x32, whole 128-byte lines
                for (u32 g = 0; g < 2; ++g)
                    for (u32 r = 0; r < 4; ++r) {
                        const u32 s = hb_mac_line_src_lane(l, g, r), lo = hb_mac_line_lane_off(l);
                        const bool ok = hb_mac_block_ok(act[s], job[s], C, len);
                        const unsigned char *a = hb_mac_src(ok, file.p, job[s], C, fb.p, lo);
                        for (u32 j0 = 0; j0 < S; j0 += 4)
                            read16("line", a, 32 * j0, full[s], file.p + job[s] * C + lo + 32 * j0, file, fb, len, S,
                                   (u32)wave, l, 4 * g + r);
                    }
            for (u32 g = 0; g < 2; ++g) {   // 32x32x32, sector-shaped loads
                const u32 s = hb_mac_sector_src_lane(l, g), lo = hb_mac_sector_lane_off(l);
                const bool ok = hb_mac_block_ok(act[s], job[s], C, len);
                const unsigned char *a = hb_mac_src(ok, file.p, job[s], C, fb.p, lo);
                for (u32 j = 0; j < S; ++j)
                    read16("sector", a, 32 * j, full[s], file.p + job[s] * C + lo + 32 * j, file, fb, len, S,
                           (u32)wave, l, g);
            }
        }
    }
}

int main() {
    const u32 Ss[] = {1, 2, 3, 4, 6, 16};
    for (u32 S : Ss) {
        const u64 C = 32ull * S;
        const u64 lens[] = {0, 1, C - 1, C, C + 1, 64 * C - 1, 65 * C + 17};
        for (u64 len : lens) sweep256(len, S);
    }
    if (g_bad) {
        printf("%lld of %lld checks failed\n", g_bad, g_checks);
        return 1;
    }
    printf("ok %lld (%u)\n", g_checks, g_sink & 1u);
    return 0;
}
