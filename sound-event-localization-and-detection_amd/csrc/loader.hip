// Device-resident epoch loader: the minibatch of a training step is gathered out of the resident dataset by a launch
// that reads WHICH batch from device memory, so the launch can be recorded once in a HIP graph and fetch the next batch
// at every replay (train.ResidentLoader, train.GraphedTrainStep).
//
//   seld_gather_rows      out[b, :] = all[index[cursor * stride + start + b], :] for the predictors and the targets
//   seld_gather_rows_aug  the same gather with the per-sample augmentation applied on the way: a signed channel
//                         permutation with the matching transform of the DOA labels, frequency and time masks
//   seld_gather_rows_rot  the same gather with a per-sample rotation of the sound field: a 3x3 matrix mixes the three
//                         channels of every intensity vector and the DOA labels, then the masks
//   seld_gather_rows_polar  the rotating gather for magnitude / phase predictors: R mixes the complex value m e^(i phi) of
//                         the three directional channels of every group (polar to Cartesian, mix, back), then the masks
//   seld_epoch_step_end   running mean of the loss, cursor += 1 (the last launch of a step)
//
// The gather is an HBM-bound copy (config 3: 2 MB per predictor row, 67 MB per batch): a row is spread over many
// workgroups in tiles of 16 KB (256 lanes x 4 x 16 bytes, all four loads issued before the first store), the grid is
// capped near 2048 workgroups and strides over the tiles beyond that.  The loads of `cursor` and `index` depend on the
// workgroup's coordinates only: the compiler keeps them on the scalar unit.  No LDS.
//
// The augmented gather moves the same bytes.  What a sample draws (Philox words of its (seed, epoch, position)) and the
// row of the transform table it picks depend on blockIdx.y only, so they are computed once per workgroup on the scalar
// unit: the channel map packed 4 bits per channel, the flips 2 bits per channel, the mask bounds as four ranges.  A
// lane then needs (c, f, t) of its output offset (two unsigned divisions by uniform divisors per 16 bytes), a shift
// for its source channel and a few compares; with T % 4 == 0 a float4 never crosses a (c, f) row.
#include "common.h"

namespace seld {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_VEC = 4;                                           // 16-byte accesses per lane and tile
constexpr long long GATHER_TILE = (long long)GATHER_THREADS * GATHER_VEC * 4;   // floats per tile
constexpr int GATHER_MAX_BLOCKS = 2048;

struct GatherSide {
    const float* all;   // (n_rows, row)
    float* out;         // (B, row)
    long long row;
};

// `len` <= GATHER_TILE floats from s to d (zeros when !valid; s is then not read).  16-byte accesses over the part where
// source and destination are 16-byte aligned TOGETHER, single floats before and behind it; when the two are aligned
// differently (a row length that is no multiple of 4 puts every other row there) the whole tile moves float by float.
__device__ __forceinline__ void gather_tile(const float* __restrict__ s, float* __restrict__ d, int len, bool valid) {
    const int tid = threadIdx.x;
    const uintptr_t da = (uintptr_t)d, sa = valid ? (uintptr_t)s : (uintptr_t)d;
    if ((da ^ sa) & 15) {
        for (int i = tid; i < len; i += GATHER_THREADS) d[i] = s[i];
        return;
    }
    int head = (int)(((16 - (da & 15)) & 15) >> 2);
    if (head > len) head = len;
    if (tid < head) d[tid] = valid ? s[tid] : 0.f;
    const int nv = (len - head) >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + head);
    float4 v[GATHER_VEC];
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        v[k] = (valid && i < nv) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        if (i < nv) d4[i] = v[k];
    }
    const int done = head + 4 * nv;
    if (tid < len - done) d[done + tid] = valid ? s[done + tid] : 0.f;
}

// grid (gx + gy, count): workgroups [0, gx) of a row copy the predictors, the rest the targets
__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_kernel(GatherSide x, GatherSide y, int gx,
                                                                     const int64_t* __restrict__ index, long long n_index,
                                                                     long long n_rows, const int32_t* __restrict__ cursor,
                                                                     long long stride, long long start) {
    const int b = blockIdx.y;
    const bool is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = is_y ? y : x;
    const int first = is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    const int step = is_y ? (int)gridDim.x - gx : gx;
    const long long p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (p >= 0 && p < n_index) r = index[p];
    const bool valid = r >= 0 && r < n_rows;        // anything else: the row is zero-filled, nothing is read
    float* dst = sd.out + (long long)b * sd.row;
    const float* src = valid ? sd.all + r * sd.row : dst;
    for (long long off = (long long)first * GATHER_TILE; off < sd.row; off += (long long)step * GATHER_TILE) {
        const long long left = sd.row - off;
        gather_tile(src + off, dst + off, (int)(left < GATHER_TILE ? left : GATHER_TILE), valid);
    }
}

// ---- augmented gather ------------------------------------------------------------------------------------------------
constexpr int AUG_MAX_C = 16, AUG_MAX_K = 64;
constexpr float PI_F = (float)M_PI;

struct AugParams {
    int C, F, T;                // predictor row = (C, F, T)
    int n_sed;                  // target row = (T_out, [n_sed activity | n_sed * 3 location])
    uint64_t seed;
    int K;                      // rows of the table (K, 2 * C + 6): src[C], flip[C], axis[3], sign[3]
    float p_swap;
    int n_fmask, f_max, n_tmask, t_max;
    float fill;
    int vec;                    // T % 4 == 0 and both predictor arrays 16-byte aligned
};

__device__ __forceinline__ uint32_t int_below(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// up to two masks over an axis of `size` from the four words of one Philox group: [lo[m], lo[m] + width[m])
struct MaskPair {
    uint32_t lo[2], width[2];
    __device__ __forceinline__ bool hit(uint32_t i) const { return (i - lo[0] < width[0]) | (i - lo[1] < width[1]); }
};
__device__ __forceinline__ MaskPair draw_masks(uint64_t counter, uint64_t seed, int n, int max_width, int size) {
    MaskPair m{{0u, 0u}, {0u, 0u}};
    if (n > 0) {
        const uint4 w = philox4x32_10(counter, seed);
        m.width[0] = int_below(w.x, (uint32_t)max_width + 1u);
        m.lo[0] = int_below(w.y, (uint32_t)size - m.width[0] + 1u);
        if (n > 1) {
            m.width[1] = int_below(w.z, (uint32_t)max_width + 1u);
            m.lo[1] = int_below(w.w, (uint32_t)size - m.width[1] + 1u);
        }
    }
    return m;
}

__device__ __forceinline__ float aug_flip(float v, uint32_t flip) {
    const float turned = v <= 0.f ? v + PI_F : v - PI_F;        // selects, no branches: the flip differs between lanes
    return flip == 1u ? -v : flip == 2u ? turned : v;
}

// what a workgroup needs of its sample's draws to place one predictor element
struct AugX {
    uint64_t src;           // 4 bits per output channel
    uint32_t flip;          // 2 bits per output channel
    MaskPair fm, tm;
    uint32_t F, T, FT;
    float fill;
};

// one predictor element at output offset o of the row
__device__ __forceinline__ float aug_x_element(const float* __restrict__ s, uint32_t o, const AugX& a) {
    const uint32_t q = o / a.T, t = o - q * a.T, c = q / a.F, f = q - c * a.F;
    if (a.fm.hit(f) || a.tm.hit(t)) return a.fill;
    const uint32_t sc = (uint32_t)(a.src >> (4u * c)) & 15u;
    return aug_flip(s[o - c * a.FT + sc * a.FT], (a.flip >> (2u * c)) & 3u);
}

// `len` <= GATHER_TILE floats (a multiple of 4) at row offset `off` (a multiple of 4), rows 16-byte aligned, T % 4 == 0:
// the four floats of an access share (c, f).  All loads of the tile are issued before its first store.
__device__ __forceinline__ void aug_x_tile_vec(const float* __restrict__ s, float* __restrict__ d, uint32_t off, int len,
                                               const AugX& a) {
    const int tid = threadIdx.x, nv = len >> 2;
    float4 v[GATHER_VEC];
    uint32_t t0[GATHER_VEC], flip[GATHER_VEC];
    bool whole[GATHER_VEC];
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        const uint32_t o = off + 4u * (uint32_t)(i < nv ? i : 0);       // a lane past the tile: any offset inside the row
        const uint32_t q = o / a.T, c = q / a.F, f = q - c * a.F;
        t0[k] = o - q * a.T;
        flip[k] = (a.flip >> (2u * c)) & 3u;
        whole[k] = a.fm.hit(f);
        const uint32_t sc = (uint32_t)(a.src >> (4u * c)) & 15u;
        v[k] = (i < nv && !whole[k]) ? *reinterpret_cast<const float4*>(s + (o - c * a.FT + sc * a.FT))
                                     : make_float4(a.fill, a.fill, a.fill, a.fill);
    }
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        if (i >= nv) continue;
        float4 r;
        r.x = (whole[k] | a.tm.hit(t0[k])) ? a.fill : aug_flip(v[k].x, flip[k]);
        r.y = (whole[k] | a.tm.hit(t0[k] + 1u)) ? a.fill : aug_flip(v[k].y, flip[k]);
        r.z = (whole[k] | a.tm.hit(t0[k] + 2u)) ? a.fill : aug_flip(v[k].z, flip[k]);
        r.w = (whole[k] | a.tm.hit(t0[k] + 3u)) ? a.fill : aug_flip(v[k].w, flip[k]);
        *reinterpret_cast<float4*>(d + off + 4u * (uint32_t)i) = r;
    }
}

// grid (gx + gy, count) as gather_rows_kernel.  Everything up to the tile loops is uniform over the workgroup; `epoch`
// and `table` are arguments of their own (not members of AugParams) so that they carry __restrict__ and their loads
// stay on the scalar unit.
// 8 waves per SIMD as gather_rows_kernel has them (the second bound keeps the scalar registers of the draws under the limit).
__global__ __launch_bounds__(GATHER_THREADS, 8) void gather_rows_aug_kernel(GatherSide x, GatherSide y, int gx,
                                                                         const int64_t* __restrict__ index, long long n_index,
                                                                         long long n_rows, const int32_t* __restrict__ cursor,
                                                                         long long stride, long long start,
                                                                         const int32_t* __restrict__ epoch,
                                                                         const int32_t* __restrict__ table, AugParams a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const bool is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = is_y ? y : x;
    const int first = is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    const int step = is_y ? (int)gridDim.x - gx : gx;
    const long long p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (p >= 0 && p < n_index) r = index[p];
    const bool valid = r >= 0 && r < n_rows;
    float* __restrict__ dst = sd.out + (long long)b * sd.row;
    const float* __restrict__ src = valid ? sd.all + r * sd.row : dst;
    const uint32_t row = (uint32_t)sd.row, first_off = (uint32_t)first * (uint32_t)GATHER_TILE;     // rows are below 2^31 floats
    const uint64_t tile_step = (uint64_t)step * (uint64_t)GATHER_TILE;

    // the draws of this sample: functions of (seed, epoch, p) alone
    uint64_t counter = 0;
    bool swap = false;
    const int32_t* __restrict__ trow = table;
    if (valid) {
        counter = ((uint64_t)(uint32_t)epoch[0] << 34) | ((uint64_t)p << 2);
        if (a.K > 0) {
            const uint4 w = philox4x32_10(counter, a.seed);
            swap = u01(w.y) < a.p_swap;
            trow += (long long)int_below(w.x, (uint32_t)a.K) * (2 * a.C + 6);
        }
    }

    // every load of the table comes before the first store of the kernel: the compiler then proves them unclobbered and
    // issues scalar loads.  Unrolled with clamped indices, so that they go out together.
    uint64_t src_map = 0xFEDCBA9876543210ull;
    uint32_t flip_map = 0u;
    int ax0 = 0, ax1 = 1, ax2 = 2;
    float sg0 = 1.f, sg1 = 1.f, sg2 = 1.f;
    if (swap && is_y) {
        // the binding validates the table; an axis outside 0..2 still reads nothing outside its own triple
        const int32_t* __restrict__ la = trow + 2 * a.C;
        ax0 = (uint32_t)la[0] < 3u ? la[0] : 0, ax1 = (uint32_t)la[1] < 3u ? la[1] : 1, ax2 = (uint32_t)la[2] < 3u ? la[2] : 2;
        sg0 = (float)la[3], sg1 = (float)la[4], sg2 = (float)la[5];
    } else if (swap) {
        uint32_t from[AUG_MAX_C], turn[AUG_MAX_C];
#pragma unroll
        for (int c = 0; c < AUG_MAX_C; ++c) {
            const int cc = c < a.C ? c : 0;
            from[c] = (uint32_t)trow[cc];
            turn[c] = (uint32_t)trow[a.C + cc];
        }
        src_map = 0ull;
#pragma unroll
        for (int c = 0; c < AUG_MAX_C; ++c) {                                       // a source outside [0, C): the channel itself
            src_map |= (uint64_t)(from[c] < (uint32_t)a.C ? from[c] : (uint32_t)(c < a.C ? c : 0)) << (4 * c);
            flip_map |= (turn[c] & 3u) << (2 * c);
        }
    }

    if (!valid || (is_y && !swap)) {            // zero-fill, or targets that no transform touches: the plain tiles
        for (uint64_t off = first_off; off < row; off += tile_step) {
            const uint32_t left = row - (uint32_t)off;
            gather_tile(src + off, dst + off, (int)(left < GATHER_TILE ? left : GATHER_TILE), valid);
        }
        return;
    }

    if (is_y) {                                 // location (s, axis) <- sign[axis] * location (s, axis[axis]); activity copied
        const uint32_t n_sed = (uint32_t)a.n_sed, cols = 4u * n_sed;
        for (uint64_t off = first_off; off < row; off += tile_step) {
            const uint32_t left = row - (uint32_t)off, len = left < GATHER_TILE ? left : (uint32_t)GATHER_TILE;
            for (uint32_t i = tid; i < len; i += GATHER_THREADS) {
                const uint32_t o = (uint32_t)off + i, j = o % cols;
                float v;
                if (j < n_sed) {
                    v = src[o];
                } else {
                    const uint32_t ax = (j - n_sed) % 3u;
                    const int from = ax == 0u ? ax0 : ax == 1u ? ax1 : ax2;
                    const float sg = ax == 0u ? sg0 : ax == 1u ? sg1 : sg2;
                    v = sg * src[o - ax + (uint32_t)from];
                }
                dst[o] = v;
            }
        }
        return;
    }

    AugX ax;
    ax.src = src_map;
    ax.flip = flip_map;
    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.F = (uint32_t)a.F;
    ax.T = (uint32_t)a.T;
    ax.FT = ax.F * ax.T;
    ax.fill = a.fill;
    for (uint64_t off = first_off; off < row; off += tile_step) {
        const uint32_t left = row - (uint32_t)off, len = left < GATHER_TILE ? left : (uint32_t)GATHER_TILE;
        if (a.vec) {
            aug_x_tile_vec(src, dst, (uint32_t)off, (int)len, ax);
        } else {
            for (uint32_t i = tid; i < len; i += GATHER_THREADS) dst[(uint32_t)off + i] = aug_x_element(src, (uint32_t)off + i, ax);
        }
    }
}

// ---- gather with a rotation of the sound field -------------------------------------------------------------------------
// Channels come in two kinds: the members of a triple (cx, cy, cz), the three components of one intensity vector, and
// the others, which pass.  A predictor row is cut into ITEMS of 16 bytes (4 bytes on the scalar path): a triple item
// is the same piece of its three channels, loaded, mixed by R and stored as three accesses; a pass item is one piece of
// one channel.  Triple items are numbered first, in tiles of ROT_TILE_A (two per lane: six 16-byte loads in flight),
// pass items behind them in tiles of ROT_TILE_B (four per lane, as the other gathers), so whether a tile mixes is
// uniform over the workgroup.  A sample that draws no rotation has pass items only: it moves as bits.
constexpr int ROT_MAX_TRIPLES = 5;
constexpr int ROT_VEC_A = 2, ROT_VEC_B = GATHER_VEC;
constexpr uint32_t ROT_TILE_A = GATHER_THREADS * ROT_VEC_A, ROT_TILE_B = GATHER_THREADS * ROT_VEC_B;     // items per tile

struct RotParams {
    int C, F, T;                // predictor row = (C, F, T)
    int n_sed;                  // target row = (T_out, [n_sed activity | n_sed * 3 location])
    uint64_t seed;
    int n_triples, n_pass;
    uint64_t triples;           // 4 bits per entry: cx, cy, cz of triple 0, of triple 1, ...
    uint64_t pass;              // 4 bits per entry: the channels outside the triples, ascending
    float p_rot;
    int mirror, zflip;
    int n_fmask, f_max, n_tmask, t_max;
    float fill;
    int vec;                    // T % 4 == 0 and both predictor arrays 16-byte aligned
};

struct RotX {
    float r[9];                 // row-major
    MaskPair fm, tm;
    uint32_t T, FT, P;          // P: items per channel
    float fill;
};

template <bool VEC> __device__ __forceinline__ float4 rot_load(const float* __restrict__ p) {
    if (VEC) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], 0.f, 0.f, 0.f);
}
template <bool VEC> __device__ __forceinline__ void rot_store(float* __restrict__ p, float4 v) {
    if (VEC) *reinterpret_cast<float4*>(p) = v;
    else p[0] = v.x;
}
__device__ __forceinline__ float rot_mix(float r0, float r1, float r2, float x, float y, float z) {
    return fmaf(r2, z, fmaf(r1, y, r0 * x));
}
__device__ __forceinline__ float4 rot_mix4(const float* __restrict__ r, float4 x, float4 y, float4 z) {
    return make_float4(rot_mix(r[0], r[1], r[2], x.x, y.x, z.x), rot_mix(r[0], r[1], r[2], x.y, y.y, z.y),
                       rot_mix(r[0], r[1], r[2], x.z, y.z, z.z), rot_mix(r[0], r[1], r[2], x.w, y.w, z.w));
}
// the time mask over the (up to) four frames of a piece that starts at frame t0; `whole`: its frequency row is masked
__device__ __forceinline__ float4 rot_masked(float4 v, bool whole, uint32_t t0, const RotX& a) {
    return make_float4((whole | a.tm.hit(t0)) ? a.fill : v.x, (whole | a.tm.hit(t0 + 1u)) ? a.fill : v.y,
                       (whole | a.tm.hit(t0 + 2u)) ? a.fill : v.z, (whole | a.tm.hit(t0 + 3u)) ? a.fill : v.w);
}

// items [first, first + ROT_TILE_A) of the n triple items: item i is piece i % P of triple i / P
template <bool VEC> __device__ __forceinline__ void rot_tile_triples(const float* __restrict__ s, float* __restrict__ d, uint32_t first,
                                                                     uint32_t n, uint64_t triples, const RotX& a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    float4 vx[ROT_VEC_A], vy[ROT_VEC_A], vz[ROT_VEC_A];
    uint32_t ox[ROT_VEC_A], oy[ROT_VEC_A], oz[ROT_VEC_A], t0[ROT_VEC_A];
    bool whole[ROT_VEC_A];
#pragma unroll
    for (int k = 0; k < ROT_VEC_A; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * GATHER_THREADS, ii = i < n ? i : 0u;    // a lane past the end: item 0
        const uint32_t u = ii / a.P, e = (ii - u * a.P) * W, f = e / a.T;
        const uint32_t m = (uint32_t)(triples >> (12u * u));
        t0[k] = e - f * a.T;
        whole[k] = a.fm.hit(f);
        ox[k] = (m & 15u) * a.FT + e, oy[k] = ((m >> 4) & 15u) * a.FT + e, oz[k] = ((m >> 8) & 15u) * a.FT + e;
        const bool load = i < n && !whole[k];
        const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
        vx[k] = load ? rot_load<VEC>(s + ox[k]) : none;
        vy[k] = load ? rot_load<VEC>(s + oy[k]) : none;
        vz[k] = load ? rot_load<VEC>(s + oz[k]) : none;
    }
#pragma unroll
    for (int k = 0; k < ROT_VEC_A; ++k) {
        if (first + threadIdx.x + (uint32_t)k * GATHER_THREADS >= n) continue;
        rot_store<VEC>(d + ox[k], rot_masked(rot_mix4(a.r, vx[k], vy[k], vz[k]), whole[k], t0[k], a));
        rot_store<VEC>(d + oy[k], rot_masked(rot_mix4(a.r + 3, vx[k], vy[k], vz[k]), whole[k], t0[k], a));
        rot_store<VEC>(d + oz[k], rot_masked(rot_mix4(a.r + 6, vx[k], vy[k], vz[k]), whole[k], t0[k], a));
    }
}

// items [first, first + ROT_TILE_B) of the n pass items: item i is piece i % P of the channel in entry i / P of `pass`
template <bool VEC> __device__ __forceinline__ void rot_tile_pass(const float* __restrict__ s, float* __restrict__ d, uint32_t first,
                                                                  uint32_t n, uint64_t pass, const RotX& a) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    float4 v[ROT_VEC_B];
    uint32_t o[ROT_VEC_B], t0[ROT_VEC_B];
    bool whole[ROT_VEC_B];
#pragma unroll
    for (int k = 0; k < ROT_VEC_B; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * GATHER_THREADS, ii = i < n ? i : 0u;
        const uint32_t u = ii / a.P, e = (ii - u * a.P) * W, f = e / a.T;
        t0[k] = e - f * a.T;
        whole[k] = a.fm.hit(f);
        o[k] = ((uint32_t)(pass >> (4u * u)) & 15u) * a.FT + e;
        v[k] = (i < n && !whole[k]) ? rot_load<VEC>(s + o[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < ROT_VEC_B; ++k) {
        if (first + threadIdx.x + (uint32_t)k * GATHER_THREADS >= n) continue;
        rot_store<VEC>(d + o[k], rot_masked(v[k], whole[k], t0[k], a));
    }
}

// the predictor row of one sample: tiles [first, ...) in steps of `step`, triple tiles before pass tiles
template <bool VEC> __device__ __forceinline__ void rot_x_row(const float* __restrict__ s, float* __restrict__ d, uint32_t first,
                                                              uint32_t step, uint32_t n_a, uint32_t n_b, uint64_t triples,
                                                              uint64_t pass, const RotX& a) {
    const uint32_t tiles_a = (n_a + ROT_TILE_A - 1u) / ROT_TILE_A, tiles_b = (n_b + ROT_TILE_B - 1u) / ROT_TILE_B;
    for (uint32_t tile = first; tile < tiles_a + tiles_b; tile += step) {
        if (tile < tiles_a) rot_tile_triples<VEC>(s, d, tile * ROT_TILE_A, n_a, triples, a);
        else rot_tile_pass<VEC>(s, d, (tile - tiles_a) * ROT_TILE_B, n_b, pass, a);
    }
}

// what a sample draws of group 3, or its explicit matrix: R (row-major) and whether it applies.  Uniform over the
// workgroup; the loads of `matrices` precede the first store of the kernel (scalar loads).
__device__ __forceinline__ bool rot_draw(bool valid, long long p, int b, const int32_t* __restrict__ epoch,
                                         const float* __restrict__ matrices, uint64_t seed, float p_rot, int mirror, int zflip,
                                         uint64_t& counter, RotX& ax) {
    float* r = ax.r;
    bool rotate = false;
    r[0] = 1.f, r[1] = 0.f, r[2] = 0.f, r[3] = 0.f, r[4] = 1.f, r[5] = 0.f, r[6] = 0.f, r[7] = 0.f, r[8] = 1.f;
    if (valid) {
        counter = ((uint64_t)(uint32_t)epoch[0] << 34) | ((uint64_t)p << 2);
        if (matrices) {
            rotate = true;
            const float* __restrict__ m = matrices + 9ll * b;
#pragma unroll
            for (int i = 0; i < 9; ++i) r[i] = m[i];
        } else if (p_rot > 0.f) {
            const uint4 w = philox4x32_10(counter | 3u, seed);
            rotate = u01(w.y) < p_rot;
            float s, c;
            sincospif(2.f * u01(w.x), &s, &c);
            const float my = (mirror && (w.z >> 31)) ? -1.f : 1.f, mz = (zflip && (w.w >> 31)) ? -1.f : 1.f;
            r[0] = c, r[1] = -s, r[3] = my * s, r[4] = my * c, r[8] = mz;
        }
    }
    return rotate;
}

// the target row of a rotated sample: location (s, a) <- sum_b R[a][b] location (s, b); activity copied
__device__ __forceinline__ void rot_y_row(const float* __restrict__ src, float* __restrict__ dst, uint32_t row, uint32_t first,
                                          uint32_t step, uint32_t n_sed, const RotX& ax) {
    // the nine entries by name: selects between values, not between addresses (an address select keeps R in memory)
    const float r00 = ax.r[0], r01 = ax.r[1], r02 = ax.r[2], r10 = ax.r[3], r11 = ax.r[4], r12 = ax.r[5], r20 = ax.r[6], r21 = ax.r[7],
                r22 = ax.r[8];
    const uint32_t cols = 4u * n_sed;
    const uint64_t tile_step = (uint64_t)step * (uint64_t)GATHER_TILE;
    for (uint64_t off = (uint64_t)first * (uint64_t)GATHER_TILE; off < row; off += tile_step) {
        const uint32_t left = row - (uint32_t)off, len = left < GATHER_TILE ? left : (uint32_t)GATHER_TILE;
        for (uint32_t i = threadIdx.x; i < len; i += GATHER_THREADS) {
            const uint32_t o = (uint32_t)off + i, j = o % cols;
            float v;
            if (j < n_sed) {
                v = src[o];
            } else {
                const uint32_t axis = (j - n_sed) % 3u, o0 = o - axis;
                const float r0 = axis == 0u ? r00 : axis == 1u ? r10 : r20;
                const float r1 = axis == 0u ? r01 : axis == 1u ? r11 : r21;
                const float r2 = axis == 0u ? r02 : axis == 1u ? r12 : r22;
                v = rot_mix(r0, r1, r2, src[o0], src[o0 + 1u], src[o0 + 2u]);
            }
            dst[o] = v;
        }
    }
}

// grid (gx + gy, count) as gather_rows_kernel.  Everything up to the tile loops is uniform over the workgroup: the draws,
// the nine entries of R (computed, or loaded from `matrices` before the first store: scalar loads), the mask bounds.
__global__ __launch_bounds__(GATHER_THREADS, 8) void gather_rows_rot_kernel(GatherSide x, GatherSide y, int gx,
                                                                         const int64_t* __restrict__ index, long long n_index,
                                                                         long long n_rows, const int32_t* __restrict__ cursor,
                                                                         long long stride, long long start,
                                                                         const int32_t* __restrict__ epoch,
                                                                         const float* __restrict__ matrices, RotParams a) {
    const int b = blockIdx.y;
    const bool is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = is_y ? y : x;
    const int first = is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    const int step = is_y ? (int)gridDim.x - gx : gx;
    const long long p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (p >= 0 && p < n_index) r = index[p];
    const bool valid = r >= 0 && r < n_rows;
    float* __restrict__ dst = sd.out + (long long)b * sd.row;
    const float* __restrict__ src = valid ? sd.all + r * sd.row : dst;
    const uint32_t row = (uint32_t)sd.row;                                  // rows are below 2^31 floats

    // the draws of this sample: functions of (seed, epoch, p) alone; an explicit matrix takes their place
    uint64_t counter = 0;
    RotX ax;
    const bool rotate = rot_draw(valid, p, b, epoch, matrices, a.seed, a.p_rot, a.mirror, a.zflip, counter, ax);

    if (!valid || (is_y && !rotate)) {          // zero-fill, or targets that no rotation touches: the plain tiles
        const uint64_t tile_step = (uint64_t)step * (uint64_t)GATHER_TILE;
        for (uint64_t off = (uint64_t)first * (uint64_t)GATHER_TILE; off < row; off += tile_step) {
            const uint32_t left = row - (uint32_t)off;
            gather_tile(src + off, dst + off, (int)(left < GATHER_TILE ? left : GATHER_TILE), valid);
        }
        return;
    }

    if (is_y) {
        rot_y_row(src, dst, row, (uint32_t)first, (uint32_t)step, (uint32_t)a.n_sed, ax);
        return;
    }

    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.T = (uint32_t)a.T;
    ax.FT = (uint32_t)a.F * ax.T;
    ax.P = a.vec ? ax.FT >> 2 : ax.FT;
    ax.fill = a.fill;
    const uint32_t n_a = rotate ? (uint32_t)a.n_triples * ax.P : 0u;
    const uint32_t n_b = (uint32_t)(rotate ? a.n_pass : a.C) * ax.P;
    const uint64_t pass = rotate ? a.pass : 0xFEDCBA9876543210ull;
    if (a.vec) rot_x_row<true>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.triples, pass, ax);
    else rot_x_row<false>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.triples, pass, ax);
}

// ---- gather with a rotation of the sound field, magnitude / phase predictors ----------------------------------------------
// Channels come as GROUPS of six, (mx, my, mz, px, py, pz): magnitude and phase of the three directional channels of one
// microphone.  A bin of the STFT is the complex number m e^(i phi) and the STFT is linear, so the rotation is the real
// matrix R applied to the complex 3-vector of every (f, t): polar to Cartesian, mix, back.  With `stats` the stored values
// are standardised, (value - mean) / sd per kind, and the kernel undoes and redoes that around the rotation.  Group
// items are numbered before pass items as the triples of gather_rows_rot_kernel are, in tiles of POLAR_TILE: one item per
// lane, six 16-byte loads in flight ahead of six stores.  sincosf (with its large-argument reduction) and atan2f, inlined
// three times each per position, fill the registers: 108 VGPRs on gfx950, so the kernel is bounded to 4 waves per SIMD
// (under the 8 of the other gathers it spills); a second item per lane would add 48 registers of data and drop to 3.
// Pass tiles, the masks, the draws and the labels are gather_rows_rot_kernel's.
constexpr int POLAR_MAX_GROUPS = 2;
constexpr int POLAR_VEC = 1;
constexpr uint32_t POLAR_TILE = GATHER_THREADS * POLAR_VEC;            // items per tile

struct PolarParams {
    int C, F, T;                // predictor row = (C, F, T)
    int n_sed;                  // target row = (T_out, [n_sed activity | n_sed * 3 location])
    uint64_t seed;
    int n_groups, n_pass;
    uint64_t groups;            // 4 bits per entry: mx, my, mz, px, py, pz of group 0, of group 1
    uint64_t pass;              // 4 bits per entry: the channels outside the groups, ascending
    float p_rot;
    int mirror, zflip;
    int n_fmask, f_max, n_tmask, t_max;
    float fill;
    int vec;                    // T % 4 == 0 and both predictor arrays 16-byte aligned
};

struct PolarStats {
    float mean_m, sd_m, mean_p, sd_p;
};

// one (f, t) of one group, in place: m[j], ph[j] (j = x, y, z) as stored -> as stored after the rotation
template <bool STATS> __device__ __forceinline__ void polar_mix(const float* __restrict__ r, const PolarStats& st, float* m, float* ph) {
#pragma clang fp contract(off)
    float re[3], im[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float mag = STATS ? fmaf(m[j], st.sd_m, st.mean_m) : m[j];
        const float phi = STATS ? fmaf(ph[j], st.sd_p, st.mean_p) : ph[j];
        float s, c;
        sincosf(phi, &s, &c);
        re[j] = mag * c;
        im[j] = mag * s;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float ra = rot_mix(r[3 * a], r[3 * a + 1], r[3 * a + 2], re[0], re[1], re[2]);
        const float ia = rot_mix(r[3 * a], r[3 * a + 1], r[3 * a + 2], im[0], im[1], im[2]);
        const float mag = sqrtf(fmaf(ia, ia, ra * ra)), phi = atan2f(ia, ra);
        m[a] = STATS ? __fdiv_rn(mag - st.mean_m, st.sd_m) : mag;
        ph[a] = STATS ? __fdiv_rn(phi - st.mean_p, st.sd_p) : phi;
    }
}

// items [first, first + POLAR_TILE) of the n group items: item i is piece i % P of group i / P
template <bool VEC, bool STATS> __device__ __forceinline__ void polar_tile_groups(const float* __restrict__ s, float* __restrict__ d,
                                                                                  uint32_t first, uint32_t n, uint64_t groups,
                                                                                  const RotX& a, const PolarStats& st) {
    constexpr uint32_t W = VEC ? 4u : 1u;
    float4 v[POLAR_VEC][6];
    uint32_t o[POLAR_VEC][6], t0[POLAR_VEC];
    bool whole[POLAR_VEC];
#pragma unroll
    for (int k = 0; k < POLAR_VEC; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * GATHER_THREADS, ii = i < n ? i : 0u;    // a lane past the end: item 0
        const uint32_t u = ii / a.P, e = (ii - u * a.P) * W, f = e / a.T;
        const uint32_t g = (uint32_t)(groups >> (24u * u));
        t0[k] = e - f * a.T;
        whole[k] = a.fm.hit(f);
        const bool load = i < n && !whole[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            o[k][j] = ((g >> (4 * j)) & 15u) * a.FT + e;
            v[k][j] = load ? rot_load<VEC>(s + o[k][j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < POLAR_VEC; ++k) {
        if (first + threadIdx.x + (uint32_t)k * GATHER_THREADS >= n) continue;
        float* lane[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) lane[j] = reinterpret_cast<float*>(&v[k][j]);
#pragma unroll
        for (int q = 0; q < (int)W; ++q) {
            float m[3] = {lane[0][q], lane[1][q], lane[2][q]}, ph[3] = {lane[3][q], lane[4][q], lane[5][q]};
            polar_mix<STATS>(a.r, st, m, ph);
#pragma unroll
            for (int j = 0; j < 3; ++j) lane[j][q] = m[j], lane[3 + j][q] = ph[j];
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) rot_store<VEC>(d + o[k][j], rot_masked(v[k][j], whole[k], t0[k], a));
    }
}

// the predictor row of one sample: tiles [first, ...) in steps of `step`, group tiles before pass tiles
template <bool VEC, bool STATS> __device__ __forceinline__ void polar_x_row(const float* __restrict__ s, float* __restrict__ d,
                                                                            uint32_t first, uint32_t step, uint32_t n_a, uint32_t n_b,
                                                                            uint64_t groups, uint64_t pass, const RotX& a,
                                                                            const PolarStats& st) {
    const uint32_t tiles_a = (n_a + POLAR_TILE - 1u) / POLAR_TILE, tiles_b = (n_b + ROT_TILE_B - 1u) / ROT_TILE_B;
    for (uint32_t tile = first; tile < tiles_a + tiles_b; tile += step) {
        if (tile < tiles_a) polar_tile_groups<VEC, STATS>(s, d, tile * POLAR_TILE, n_a, groups, a, st);
        else rot_tile_pass<VEC>(s, d, (tile - tiles_a) * ROT_TILE_B, n_b, pass, a);
    }
}

// grid (gx + gy, count) as gather_rows_kernel.  Uniform over the workgroup as in gather_rows_rot_kernel; the four
// statistics are loaded before the first store as well (one scalar load).
__global__ __launch_bounds__(GATHER_THREADS, 4) void gather_rows_polar_kernel(GatherSide x, GatherSide y, int gx,
                                                                           const int64_t* __restrict__ index, long long n_index,
                                                                           long long n_rows, const int32_t* __restrict__ cursor,
                                                                           long long stride, long long start,
                                                                           const int32_t* __restrict__ epoch,
                                                                           const float* __restrict__ matrices,
                                                                           const float* __restrict__ stats, PolarParams a) {
    const int b = blockIdx.y;
    const bool is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = is_y ? y : x;
    const int first = is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    const int step = is_y ? (int)gridDim.x - gx : gx;
    const long long p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (p >= 0 && p < n_index) r = index[p];
    const bool valid = r >= 0 && r < n_rows;
    float* __restrict__ dst = sd.out + (long long)b * sd.row;
    const float* __restrict__ src = valid ? sd.all + r * sd.row : dst;
    const uint32_t row = (uint32_t)sd.row;                                  // rows are below 2^31 floats

    uint64_t counter = 0;
    RotX ax;
    const bool rotate = rot_draw(valid, p, b, epoch, matrices, a.seed, a.p_rot, a.mirror, a.zflip, counter, ax);
    PolarStats st{0.f, 1.f, 0.f, 1.f};
    if (stats && rotate && !is_y) st = PolarStats{stats[0], stats[1], stats[2], stats[3]};

    if (!valid || (is_y && !rotate)) {          // zero-fill, or targets that no rotation touches: the plain tiles
        const uint64_t tile_step = (uint64_t)step * (uint64_t)GATHER_TILE;
        for (uint64_t off = (uint64_t)first * (uint64_t)GATHER_TILE; off < row; off += tile_step) {
            const uint32_t left = row - (uint32_t)off;
            gather_tile(src + off, dst + off, (int)(left < GATHER_TILE ? left : GATHER_TILE), valid);
        }
        return;
    }

    if (is_y) {
        rot_y_row(src, dst, row, (uint32_t)first, (uint32_t)step, (uint32_t)a.n_sed, ax);
        return;
    }

    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.T = (uint32_t)a.T;
    ax.FT = (uint32_t)a.F * ax.T;
    ax.P = a.vec ? ax.FT >> 2 : ax.FT;
    ax.fill = a.fill;
    const uint32_t n_a = rotate ? (uint32_t)a.n_groups * ax.P : 0u;
    const uint32_t n_b = (uint32_t)(rotate ? a.n_pass : a.C) * ax.P;
    const uint64_t pass = rotate ? a.pass : 0xFEDCBA9876543210ull;
    if (stats) {
        if (a.vec) polar_x_row<true, true>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.groups, pass, ax, st);
        else polar_x_row<false, true>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.groups, pass, ax, st);
    } else {
        if (a.vec) polar_x_row<true, false>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.groups, pass, ax, st);
        else polar_x_row<false, false>(src, dst, (uint32_t)first, (uint32_t)step, n_a, n_b, a.groups, pass, ax, st);
    }
}

// one thread: the epoch loop's running mean (train.main), `mean += (loss - mean) / (i + 1)` in fp32 with i the cursor,
// then the cursor
__global__ void epoch_step_end_kernel(const float* __restrict__ loss, float* __restrict__ mean, int32_t* __restrict__ cursor) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t c = cursor[0];
        const float m = mean[0];
        mean[0] = m + (loss[0] - m) / (float)(c + 1);
        cursor[0] = c + 1;
    }
}

}  // namespace seld

using namespace seld;

extern "C" int seld_gather_rows(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                int64_t cursor_stride, int64_t start, int32_t B, int32_t count, void* stream) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (!index || n_index <= 0 || n_rows <= 0 || B <= 0 || count <= 0 || count > B || count > 65535) return SELD_EINVAL;
    if (!has_x && !has_y) return SELD_EINVAL;
    if (has_x && (!x_all || !out_x || row_x <= 0)) return SELD_EINVAL;
    if (has_y && (!y_all || !out_y || row_y <= 0)) return SELD_EINVAL;
    if (cursor && cursor_stride < 0) return SELD_EINVAL;
    const long long cap = GATHER_MAX_BLOCKS / count > 0 ? GATHER_MAX_BLOCKS / count : 1;
    const long long tx = has_x ? (row_x + GATHER_TILE - 1) / GATHER_TILE : 0, ty = has_y ? (row_y + GATHER_TILE - 1) / GATHER_TILE : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{x_all, out_x, has_x ? (long long)row_x : 0}, y{y_all, out_y, has_y ? (long long)row_y : 0};
    hipLaunchKernelGGL(gather_rows_kernel, dim3(gx + gy, count), dim3(GATHER_THREADS), 0, (hipStream_t)stream, x, y, gx, index,
                       (long long)n_index, (long long)n_rows, cursor, (long long)cursor_stride, (long long)start);
    return check_launch();
}

// what seld_gather_rows_aug and seld_gather_rows_rot refuse (SELD_EINVAL) of the arguments they share
static bool aug_gather_refused(const float* x_all, int64_t row_x, const float* out_x, const float* y_all, int64_t row_y,
                               const float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                               int64_t cursor_stride, int32_t B, int32_t count, int32_t C, int32_t F, int32_t T, int32_t y_cols,
                               const int32_t* epoch, int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (!index || n_index <= 0 || n_index > (1ll << 32) || n_rows <= 0 || B <= 0 || count <= 0 || count > B || count > 65535) return true;
    if (!has_x && !has_y) return true;
    if (has_x && (!x_all || !out_x || row_x <= 0)) return true;
    if (has_y && (!y_all || !out_y || row_y <= 0)) return true;
    if (cursor && cursor_stride < 0) return true;
    if (!epoch || C < 1 || C > AUG_MAX_C || F < 1 || T < 1) return true;
    if (n_fmask < 0 || n_fmask > 2 || n_tmask < 0 || n_tmask > 2 || f_max < 0 || f_max > F || t_max < 0 || t_max > T) return true;
    if (has_x && (long long)C * F * T != row_x) return true;                        // 16 * 2^31 * 2^31 fits an int64
    return has_y && (y_cols < 4 || y_cols % 4 || row_y % y_cols);
}

// `n` (at most 15) channel entries packed 4 bits each: refused unless they are distinct, inside [0, C) and the bits above
// them 0.  `pass` receives the other channels of [0, C), ascending, packed the same way.
static bool packed_channels_refused(uint64_t packed, int n, int C, uint64_t& pass, int& n_pass) {
    uint32_t used = 0u;
    for (int i = 0; i < n; ++i) {
        const uint32_t c = (uint32_t)(packed >> (4 * i)) & 15u;
        if (c >= (uint32_t)C || (used >> c & 1u)) return true;
        used |= 1u << c;
    }
    if ((packed >> (4 * n)) != 0) return true;
    pass = 0;
    n_pass = 0;
    for (int c = 0; c < C; ++c)
        if (!(used >> c & 1u)) pass |= (uint64_t)c << (4 * n_pass++);
    return false;
}

extern "C" int seld_gather_rows_aug(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                    float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                    int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                    int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, const int32_t* table,
                                    int32_t K, float p_swap, int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max,
                                    float fill, void* stream) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (aug_gather_refused(x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, B, count, C, F, T,
                           y_cols, epoch, n_fmask, f_max, n_tmask, t_max))
        return SELD_EINVAL;
    if (K < 0 || K > AUG_MAX_K || (K > 0) != (table != nullptr)) return SELD_EINVAL;
    if (!(p_swap >= 0.f && p_swap <= 1.f)) return SELD_EINVAL;                      // a NaN fails both
    if (row_x >= (1ll << 31) || row_y >= (1ll << 31)) return SELD_EUNSUPPORTED;     // offsets inside a row are 32-bit
    const long long cap = GATHER_MAX_BLOCKS / count > 0 ? GATHER_MAX_BLOCKS / count : 1;
    const long long tx = has_x ? (row_x + GATHER_TILE - 1) / GATHER_TILE : 0, ty = has_y ? (row_y + GATHER_TILE - 1) / GATHER_TILE : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{x_all, out_x, has_x ? (long long)row_x : 0}, y{y_all, out_y, has_y ? (long long)row_y : 0};
    const int vec = has_x && T % 4 == 0 && (((uintptr_t)x_all | (uintptr_t)out_x) & 15) == 0;
    const AugParams a{C, F, T, has_y ? y_cols / 4 : 0, seed, K, p_swap, n_fmask, f_max, n_tmask, t_max, fill, vec};
    hipLaunchKernelGGL(gather_rows_aug_kernel, dim3(gx + gy, count), dim3(GATHER_THREADS), 0, (hipStream_t)stream, x, y, gx, index,
                       (long long)n_index, (long long)n_rows, cursor, (long long)cursor_stride, (long long)start, epoch, table, a);
    return check_launch();
}

extern "C" int seld_gather_rows_rot(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                    float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                    int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                    int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, uint64_t triples,
                                    int32_t n_triples, float p_rot, int32_t rot_mirror, int32_t rot_zflip, const float* matrices,
                                    int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max, float fill, void* stream) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (aug_gather_refused(x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, B, count, C, F, T,
                           y_cols, epoch, n_fmask, f_max, n_tmask, t_max))
        return SELD_EINVAL;
    if (n_triples < 1 || n_triples > ROT_MAX_TRIPLES || 3 * n_triples > C) return SELD_EINVAL;
    if (!(p_rot >= 0.f && p_rot <= 1.f)) return SELD_EINVAL;                        // a NaN fails both
    if (row_x >= (1ll << 31) || row_y >= (1ll << 31)) return SELD_EUNSUPPORTED;     // offsets inside a row are 32-bit
    // the triples travel by value, so their content is checked here: the kernel then indexes with them as they are
    uint64_t pass = 0;
    int n_pass = 0;
    if (packed_channels_refused(triples, 3 * n_triples, C, pass, n_pass)) return SELD_EINVAL;      // at most 60 bits are entries
    const int vec = has_x && T % 4 == 0 && (((uintptr_t)x_all | (uintptr_t)out_x) & 15) == 0;
    // the grid of seld_gather_rows_aug over the tiles of this kernel: the larger of a rotated and an unrotated sample's
    const long long P = has_x ? (vec ? (long long)F * T / 4 : (long long)F * T) : 0;
    const long long cap = GATHER_MAX_BLOCKS / count > 0 ? GATHER_MAX_BLOCKS / count : 1;
    const long long t_rot = (n_triples * P + ROT_TILE_A - 1) / ROT_TILE_A + (n_pass * P + ROT_TILE_B - 1) / ROT_TILE_B;
    const long long t_plain = (C * P + ROT_TILE_B - 1) / ROT_TILE_B;
    const long long tx = t_rot > t_plain ? t_rot : t_plain;
    const long long ty = has_y ? (row_y + GATHER_TILE - 1) / GATHER_TILE : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{x_all, out_x, has_x ? (long long)row_x : 0}, y{y_all, out_y, has_y ? (long long)row_y : 0};
    const RotParams a{C, F, T, has_y ? y_cols / 4 : 0, seed, n_triples, n_pass, triples, pass, p_rot, rot_mirror != 0, rot_zflip != 0,
                      n_fmask, f_max, n_tmask, t_max, fill, vec};
    hipLaunchKernelGGL(gather_rows_rot_kernel, dim3(gx + gy, count), dim3(GATHER_THREADS), 0, (hipStream_t)stream, x, y, gx, index,
                       (long long)n_index, (long long)n_rows, cursor, (long long)cursor_stride, (long long)start, epoch, matrices, a);
    return check_launch();
}

extern "C" int seld_gather_rows_polar(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                      float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                      int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                      int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, uint64_t groups,
                                      int32_t n_groups, const float* stats, float p_rot, int32_t rot_mirror, int32_t rot_zflip,
                                      const float* matrices, int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max,
                                      float fill, void* stream) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (aug_gather_refused(x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, B, count, C, F, T,
                           y_cols, epoch, n_fmask, f_max, n_tmask, t_max))
        return SELD_EINVAL;
    if (n_groups < 1 || n_groups > POLAR_MAX_GROUPS || 6 * n_groups > C) return SELD_EINVAL;
    if (!(p_rot >= 0.f && p_rot <= 1.f)) return SELD_EINVAL;                        // a NaN fails both
    if (row_x >= (1ll << 31) || row_y >= (1ll << 31)) return SELD_EUNSUPPORTED;     // offsets inside a row are 32-bit
    // the groups travel by value, so their content is checked here: the kernel then indexes with them as they are
    uint64_t pass = 0;
    int n_pass = 0;
    if (packed_channels_refused(groups, 6 * n_groups, C, pass, n_pass)) return SELD_EINVAL;        // at most 48 bits are entries
    const int vec = has_x && T % 4 == 0 && (((uintptr_t)x_all | (uintptr_t)out_x) & 15) == 0;
    // the grid of seld_gather_rows_rot over the tiles of this kernel: the larger of a rotated and an unrotated sample's
    const long long P = has_x ? (vec ? (long long)F * T / 4 : (long long)F * T) : 0;
    const long long cap = GATHER_MAX_BLOCKS / count > 0 ? GATHER_MAX_BLOCKS / count : 1;
    const long long t_rot = (n_groups * P + POLAR_TILE - 1) / POLAR_TILE + (n_pass * P + ROT_TILE_B - 1) / ROT_TILE_B;
    const long long t_plain = (C * P + ROT_TILE_B - 1) / ROT_TILE_B;
    const long long tx = t_rot > t_plain ? t_rot : t_plain;
    const long long ty = has_y ? (row_y + GATHER_TILE - 1) / GATHER_TILE : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{x_all, out_x, has_x ? (long long)row_x : 0}, y{y_all, out_y, has_y ? (long long)row_y : 0};
    const PolarParams a{C, F, T, has_y ? y_cols / 4 : 0, seed, n_groups, n_pass, groups, pass, p_rot, rot_mirror != 0, rot_zflip != 0,
                        n_fmask, f_max, n_tmask, t_max, fill, vec};
    hipLaunchKernelGGL(gather_rows_polar_kernel, dim3(gx + gy, count), dim3(GATHER_THREADS), 0, (hipStream_t)stream, x, y, gx, index,
                       (long long)n_index, (long long)n_rows, cursor, (long long)cursor_stride, (long long)start, epoch, matrices, stats,
                       a);
    return check_launch();
}

extern "C" int seld_epoch_step_end(const float* loss, float* mean, int32_t* cursor, void* stream) {
    if (!loss || !mean || !cursor) return SELD_EINVAL;
    hipLaunchKernelGGL(epoch_step_end_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, mean, cursor);
    return check_launch();
}
