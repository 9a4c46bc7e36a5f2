// What the kernels that apply a row of the FOA transform table to predictors share (loader.hip: gather_rows_aug_kernel;
// ensemble.hip: window_batch_kernel): the tile geometry, the packed channel map of a row, and flipop.
#pragma once
#include "common.h"

namespace seld {

// a row is spread over workgroups in tiles of 16 KB (256 lanes x 4 x 16 bytes, every load of a tile issued before its first
// store); the grid is capped near 2048 workgroups and strides over the tiles beyond that
constexpr int TILE_THREADS = 256;
constexpr int TILE_VEC = 4;                                             // 16-byte accesses per lane and tile
constexpr uint32_t TILE_FLOATS = (uint32_t)TILE_THREADS * TILE_VEC * 4;
constexpr int TILE_MAX_BLOCKS = 2048;
constexpr int MAP_MAX_C = 16, MAP_MAX_K = 64;                           // channels and rows of a transform table
constexpr float PI_F = (float)M_PI;

// flipop of seld_gather_rows_aug: 0 keeps, 1 negates, 2 turns a phase by pi
__device__ __forceinline__ float flipop(float v, uint32_t flip) {
    const float turned = v <= 0.f ? v + PI_F : v - PI_F;                // selects, no branches: the flip differs between lanes
    return flip == 1u ? -v : flip == 2u ? turned : v;
}

// src[C], flip[C] of a table row: 4 bits of source per output channel, 2 bits of flip
struct ChannelMap {
    uint64_t src = 0xFEDCBA9876543210ull;                               // the identity
    uint32_t flip = 0u;
    __device__ __forceinline__ uint32_t source(uint32_t c) const { return (uint32_t)(src >> (4u * c)) & 15u; }
    __device__ __forceinline__ uint32_t flip_of(uint32_t c) const { return (flip >> (2u * c)) & 3u; }
};

// The map of the row at `trow` (2 * C + 6 ints).  Called ahead of the first store of a kernel, with `trow` derived from a
// __restrict__ kernel argument: the compiler then proves the loads unclobbered and issues scalar loads.  Unrolled with
// clamped indices, so that they go out together.  The bindings validate the table; a source outside [0, C) still maps
// the channel to itself.
__device__ __forceinline__ ChannelMap load_channel_map(const int32_t* __restrict__ trow, int C) {
    uint32_t from[MAP_MAX_C], turn[MAP_MAX_C];
#pragma unroll
    for (int c = 0; c < MAP_MAX_C; ++c) {
        const int cc = c < C ? c : 0;
        from[c] = (uint32_t)trow[cc];
        turn[c] = (uint32_t)trow[C + cc];
    }
    ChannelMap m;
    m.src = 0ull;
#pragma unroll
    for (int c = 0; c < MAP_MAX_C; ++c) {
        m.src |= (uint64_t)(from[c] < (uint32_t)C ? from[c] : (uint32_t)(c < C ? c : 0)) << (4 * c);
        m.flip |= (turn[c] & 3u) << (2 * c);
    }
    return m;
}

}  // namespace seld
