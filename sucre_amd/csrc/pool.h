// Pooled radix select: exact order statistics of the valid pixels of MANY images -- of any sizes, possibly spread over
// several ranks -- without concatenating or moving them (include/sucre_hip.h, sucre_pool_select_*).
//
// The select of plot.hip (most significant byte first, four passes of 256-bin histograms over order_key) split into its
// phases, so that the host can add the histograms of other chunks and other ranks between them:
//   begin    zeroes the state
//   pass     ADDS the histogram of key byte 3 - pass of a chunk of images, for the keys whose higher bytes equal the rank's prefix
//   locate   consumes the histograms: the byte under which every rank falls, the new prefix, the rank among the keys that
//            share it; zeroes the histograms; after pass 3 the prefix is the key of the value
// Pass 0 has no prefix yet, so its histogram ([c][0]) counts every valid pixel once: its sum IS the pooled valid count, and
// the host forms the ranks from it before the first locate.  Global counts are 64-bit (a pool may pass 2^32 pixels); a
// workgroup's LDS counts are 32-bit (it sees kPoolBlockPx pixels).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sucre {

constexpr int kPoolMaxRanks = 8;
constexpr int kPoolMaxImages = 4096;        // images per sucre_pool_select_pass call (the table's bisection: 12 steps)
constexpr int kPoolGroupsPerLane = 16;      // 4-pixel groups a lane walks: one LDS histogram per 16384 pixels
constexpr uint32_t kPoolBlockPx = 256u * 4u * kPoolGroupsPerLane;

struct PoolState {
    uint64_t hist[3][kPoolMaxRanks][256];   // FIRST, by contract: the host all-reduces these 6144 words; pass 0 uses [c][0]
    uint64_t remaining[3][kPoolMaxRanks];   // rank among the keys that share the prefix
    uint32_t prefix[3][kPoolMaxRanks];      // key bytes fixed so far, right-aligned
};

struct PoolImage {     // the device table's entry
    const float *J;    // (n_px, 3) float32, 16-byte aligned
    int64_t n_px;
    uint32_t block0;   // the image's first workgroup in the launch grid
    uint32_t pad;
};

inline uint64_t pool_blocks(int64_t n_px) { return ((uint64_t)n_px + kPoolBlockPx - 1) / kPoolBlockPx; }

}  // namespace sucre
