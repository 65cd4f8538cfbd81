// hb_mac_src.hpp -- where the 256-bit matrix-core MACs (hb_kernels.hpp:
// hb_mfma_block_acc, hb_mfma16_block_acc) read their 16-byte pieces of the
// file from.
//
// Every piece is loaded UNCONDITIONALLY and zeroed afterwards where its lane
// has no block: written as `ok ? *ptr : 0` each load became a divergent branch
// of its own that ended in s_waitcnt vmcnt(0) (the compiler sinks the -128
// shift into the branch), so the loads of a round went out one at a time, one
// memory round trip each.  A lane without a block (an idle
// lane of the last wave, the short last block, a file shorter than a block)
// therefore needs an address that is valid device memory whatever the file
// holds: the MAC's own A-fragment buffer, which exists whenever the MAC runs
// and is at least 32x the block size (hb_mac_fallback_bytes).
//
// Compiles as HIP device code and as plain C++: tests/macsrc/addr_main.cpp
// sweeps file lengths, sector counts, lanes and K slices and checks every
// address against the two buffers.
#pragma once
#include <stdint.h>

#ifndef HB_HD   // (as in hb_lane.hpp)
#if defined(__HIP__)
#define HB_HD __device__ __forceinline__
#else
#define HB_HD static inline
#endif
#endif

typedef uint32_t u32;
typedef uint64_t u64;

// the block `job` of an active lane lies wholly inside the data
HB_HD bool hb_mac_block_ok(bool active, u64 job, u64 C, u64 len) { return active && (job + 1) * C <= len; }

// Bytes of the A-fragment buffer of the 256-bit MAC (hb_runtime.cpp,
// mfma_tables): 64 lanes x 16 bytes per sector and tile.  A lane's loads
// cover [lane_off + step, + 16) with lane_off + step + 16 <= C = 32 S.
HB_HD u64 hb_mac_fallback_bytes(u32 S, u32 ntiles) { return (u64)ntiles * S * 64u * 16u; }

// First byte a lane's loads of one block are relative to: byte `lane_off` of
// block jb of the file (ok), else byte `lane_off` of the fallback buffer.
// The same step offsets (< C - lane_off) are then added to either.
HB_HD const unsigned char *hb_mac_src(bool ok, const unsigned char *data, u64 jb, u64 C, const unsigned char *fb,
                                      u32 lane_off) {
    return (ok ? data + jb * C : fb) + lane_off;
}

// lane_off of the three 256-bit layouts (lane l of the wave):
//   16x16x64 (EncodeArgs::mfma == 3): bytes 16 q .. of the 64-byte K slice, q = l >> 4
//   32x32x32 whole-line loads (2):    chunk 4 h + i of the 128-byte line, h = l >> 5, i = l & 3
//   32x32x32 sector loads (1):        half h of the 32-byte sector
HB_HD u32 hb_mac16_lane_off(u32 l) { return 16u * (l >> 4); }
HB_HD u32 hb_mac_line_lane_off(u32 l) { return 64u * (l >> 5) + 16u * (l & 3u); }
HB_HD u32 hb_mac_sector_lane_off(u32 l) { return 16u * (l >> 5); }
// ... and the lane whose block lane l reads in its load g (16x16x64: group
// g < 4; whole-line: group g < 2, load r < 4; sector: group g < 2)
HB_HD u32 hb_mac16_src_lane(u32 l, u32 g) { return 16u * g + (l & 15u); }
HB_HD u32 hb_mac_line_src_lane(u32 l, u32 g, u32 r) { return 32u * g + (l & 28u) + r; }
HB_HD u32 hb_mac_sector_src_lane(u32 l, u32 g) { return 32u * g + (l & 31u); }
