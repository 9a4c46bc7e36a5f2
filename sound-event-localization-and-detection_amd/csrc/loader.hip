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
//   seld_gather_rows_mix  the gather that mixes a second clip into a sample, for magnitude / phase predictors: the complex
//                         sum z_A + g z_B per bin, the track slots of both targets packed per (frame, class), then the masks
//   seld_target_occupancy per resident target row and class the most slots active in one frame (what the mix consults)
//   seld_epoch_step_end   running mean of the loss, cursor += 1 (the last launch of a step)
//
// The gather is an HBM-bound copy (config 3: 2 MB per predictor row, 67 MB per batch): a row is spread over many
// workgroups in tiles of 16 KB (channel_map.h has the geometry, shared with ensemble.hip), the grid is capped near 2048
// workgroups and strides over the tiles beyond that.  No LDS.
//
// How the four kernels are put together.  Each starts with the same preamble, `resolve_row`: which side, which tiles and
// which resident row a workgroup has, from its coordinates, `cursor` and `index` alone, so the compiler keeps those loads
// on the scalar unit.  Rows that nothing transforms (zero rows, targets of an untransformed sample, everything in
// gather_rows_kernel) go through one copy loop, `plain_row`.  What a sample draws are Philox words of its
// `sample_counter` (seed, epoch, position): they depend on blockIdx.y only and are computed once per workgroup on the
// scalar unit, as are the mask bounds (four ranges) and, in the augmented gather, the channel map of the table row.
// The two rotating kernels are ONE body, `rot_gather`, instantiated with the kind of tile that mixes: channel triples
// (gather_rows_rot_kernel) or magnitude / phase groups with their statistics (gather_rows_polar_kernel); the draw of R,
// the label rows, the masks, the pass tiles and the walk over "mixing tiles, then pass tiles" are the body's.
// gather_rows_mix_kernel has the preamble, the masks, the items and the pass tiles of the rotating kernels, a draw of its
// own (a partner and a gain under another Philox key) and a second source row on both sides.
//
// Two things that look alike stay apart on purpose: the signed permutation of gather_rows_aug_kernel (labels sign * v,
// channels moved and flipped) and the 3x3 matrix of the rotating kernels (fmaf(r2, z, fmaf(r1, y, r0 * x))).  A
// permutation matrix through the fma chain gives another sign of zero and 0 * inf = NaN beside a non-finite neighbour;
// include/seld_hip.h specifies each formula as it is.
#include "channel_map.h"

namespace seld {

struct GatherSide {
    const float* all;   // (n_rows, row)
    float* out;         // (B, row)
    long long row;
};

// `len` <= TILE_FLOATS floats from s to d (zeros when !valid; s is then not read).  16-byte accesses over the part where
// source and destination are 16-byte aligned TOGETHER, single floats before and behind it; when the two are aligned
// differently (a row length that is no multiple of 4 puts every other row there) the whole tile moves float by float.
__device__ __forceinline__ void gather_tile(const float* __restrict__ s, float* __restrict__ d, int len, bool valid) {
    const int tid = threadIdx.x;
    const uintptr_t da = (uintptr_t)d, sa = valid ? (uintptr_t)s : (uintptr_t)d;
    if ((da ^ sa) & 15) {
        for (int i = tid; i < len; i += TILE_THREADS) d[i] = s[i];
        return;
    }
    int head = (int)(((16 - (da & 15)) & 15) >> 2);
    if (head > len) head = len;
    if (tid < head) d[tid] = valid ? s[tid] : 0.f;
    const int nv = (len - head) >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + head);
    float4 v[TILE_VEC];
#pragma unroll
    for (int k = 0; k < TILE_VEC; ++k) {
        const int i = tid + k * TILE_THREADS;
        v[k] = (valid && i < nv) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < TILE_VEC; ++k) {
        const int i = tid + k * TILE_THREADS;
        if (i < nv) d4[i] = v[k];
    }
    const int done = head + 4 * nv;
    if (tid < len - done) d[done + tid] = valid ? s[done + tid] : 0.f;
}

// What a workgroup of the grid (gx + gy, count) has to do: workgroups [0, gx) of a row copy the predictors, the rest the
// targets; a side's workgroup `first` takes the tiles first, first + step, ... of batch row blockIdx.y.
struct GatherRow {
    bool is_y, valid;           // valid: the position and its index exist; anything else is zero-filled, nothing is read
    int first, step;
    long long p, r, row;        // position in `index`, the resident row it names (when valid); floats in a row of this side
    const float* src;           // the resident row (dst when !valid)
    float* dst;
};

// `index` and `cursor` are __restrict__ arguments of the kernels, and their loads depend on the workgroup's coordinates
// only and precede every store: scalar loads.
__device__ __forceinline__ GatherRow resolve_row(const GatherSide& x, const GatherSide& y, int gx, const int64_t* __restrict__ index,
                                                 long long n_index, long long n_rows, const int32_t* __restrict__ cursor,
                                                 long long stride, long long start) {
    GatherRow w;
    const int b = blockIdx.y;
    w.is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = w.is_y ? y : x;
    w.first = w.is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    w.step = w.is_y ? (int)gridDim.x - gx : gx;
    w.p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (w.p >= 0 && w.p < n_index) r = index[w.p];
    w.valid = r >= 0 && r < n_rows;
    w.r = r;
    w.row = sd.row;
    w.dst = sd.out + (long long)b * sd.row;
    w.src = w.valid ? sd.all + r * sd.row : w.dst;
    return w;
}

// the tiles of a row that only moves (or is zero-filled); 64-bit offsets: the plain gather takes rows of 2^31 floats and more
__device__ __forceinline__ void plain_row(const GatherRow& w) {
    for (long long off = (long long)w.first * TILE_FLOATS; off < w.row; off += (long long)w.step * TILE_FLOATS) {
        const long long left = w.row - off;
        gather_tile(w.src + off, w.dst + off, (int)(left < TILE_FLOATS ? left : TILE_FLOATS), w.valid);
    }
}

__global__ __launch_bounds__(TILE_THREADS) void gather_rows_kernel(GatherSide x, GatherSide y, int gx,
                                                                   const int64_t* __restrict__ index, long long n_index,
                                                                   long long n_rows, const int32_t* __restrict__ cursor,
                                                                   long long stride, long long start) {
    plain_row(resolve_row(x, y, gx, index, n_index, n_rows, cursor, stride, start));
}

// ---- what the three augmenting gathers share -----------------------------------------------------------------------------
struct AugParams {
    int C, F, T;                // predictor row = (C, F, T)
    int n_sed;                  // target row = (T_out, [n_sed activity | n_sed * 3 location])
    uint64_t seed;
    int n_fmask, f_max, n_tmask, t_max;
    float fill;
    int vec;                    // T % 4 == 0 and both predictor arrays 16-byte aligned
};

// The Philox counter of the sample at position p: its draws are functions of (seed, epoch, p) alone; the two low bits
// number the group of four words.  `epoch` is a __restrict__ argument of the kernels: a scalar load.
__device__ __forceinline__ uint64_t sample_counter(const int32_t* __restrict__ epoch, long long p) {
    return ((uint64_t)(uint32_t)epoch[0] << 34) | ((uint64_t)p << 2);
}

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

// ---- augmented gather ------------------------------------------------------------------------------------------------
// A lane needs (c, f, t) of its output offset (two unsigned divisions by uniform divisors per 16 bytes), a shift for its
// source channel and a few compares; with T % 4 == 0 a float4 never crosses a (c, f) row.

// what a workgroup needs of its sample's draws to place one predictor element
struct AugX {
    ChannelMap map;
    MaskPair fm, tm;
    uint32_t F, T, FT;
    float fill;
};

// one predictor element at output offset o of the row
__device__ __forceinline__ float aug_x_element(const float* __restrict__ s, uint32_t o, const AugX& a) {
    const uint32_t q = o / a.T, t = o - q * a.T, c = q / a.F, f = q - c * a.F;
    if (a.fm.hit(f) || a.tm.hit(t)) return a.fill;
    return flipop(s[o - c * a.FT + a.map.source(c) * a.FT], a.map.flip_of(c));
}

// `len` <= TILE_FLOATS floats (a multiple of 4) at row offset `off` (a multiple of 4), rows 16-byte aligned, T % 4 == 0:
// the four floats of an access share (c, f).  All loads of the tile are issued before its first store.
__device__ __forceinline__ void aug_x_tile_vec(const float* __restrict__ s, float* __restrict__ d, uint32_t off, int len,
                                               const AugX& a) {
    const int tid = threadIdx.x, nv = len >> 2;
    float4 v[TILE_VEC];
    uint32_t t0[TILE_VEC], flip[TILE_VEC];
    bool whole[TILE_VEC];
#pragma unroll
    for (int k = 0; k < TILE_VEC; ++k) {
        const int i = tid + k * TILE_THREADS;
        const uint32_t o = off + 4u * (uint32_t)(i < nv ? i : 0);       // a lane past the tile: any offset inside the row
        const uint32_t q = o / a.T, c = q / a.F, f = q - c * a.F;
        t0[k] = o - q * a.T;
        flip[k] = a.map.flip_of(c);
        whole[k] = a.fm.hit(f);
        v[k] = (i < nv && !whole[k]) ? *reinterpret_cast<const float4*>(s + (o - c * a.FT + a.map.source(c) * a.FT))
                                     : make_float4(a.fill, a.fill, a.fill, a.fill);
    }
#pragma unroll
    for (int k = 0; k < TILE_VEC; ++k) {
        const int i = tid + k * TILE_THREADS;
        if (i >= nv) continue;
        float4 r;
        r.x = (whole[k] | a.tm.hit(t0[k])) ? a.fill : flipop(v[k].x, flip[k]);
        r.y = (whole[k] | a.tm.hit(t0[k] + 1u)) ? a.fill : flipop(v[k].y, flip[k]);
        r.z = (whole[k] | a.tm.hit(t0[k] + 2u)) ? a.fill : flipop(v[k].z, flip[k]);
        r.w = (whole[k] | a.tm.hit(t0[k] + 3u)) ? a.fill : flipop(v[k].w, flip[k]);
        *reinterpret_cast<float4*>(d + off + 4u * (uint32_t)i) = r;
    }
}

// grid (gx + gy, count).  Everything up to the tile loops is uniform over the workgroup; `epoch` and `table` are
// arguments of their own (not members of a struct) so that they carry __restrict__ and their loads stay on the scalar
// unit.  K rows in the table (K, 2 * C + 6): src[C], flip[C], axis[3], sign[3].
// 8 waves per SIMD as gather_rows_kernel has them (the second bound keeps the scalar registers of the draws under the limit).
__global__ __launch_bounds__(TILE_THREADS, 8) void gather_rows_aug_kernel(GatherSide x, GatherSide y, int gx,
                                                                       const int64_t* __restrict__ index, long long n_index,
                                                                       long long n_rows, const int32_t* __restrict__ cursor,
                                                                       long long stride, long long start,
                                                                       const int32_t* __restrict__ epoch,
                                                                       const int32_t* __restrict__ table, AugParams a, int K,
                                                                       float p_swap) {
    const GatherRow w = resolve_row(x, y, gx, index, n_index, n_rows, cursor, stride, start);
    const int tid = threadIdx.x;
    float* __restrict__ dst = w.dst;
    const float* __restrict__ src = w.src;
    const uint32_t row = (uint32_t)w.row, first_off = (uint32_t)w.first * TILE_FLOATS;      // rows are below 2^31 floats
    const uint64_t tile_step = (uint64_t)w.step * (uint64_t)TILE_FLOATS;

    // the draws of this sample
    uint64_t counter = 0;
    bool swap = false;
    const int32_t* __restrict__ trow = table;
    if (w.valid) {
        counter = sample_counter(epoch, w.p);
        if (K > 0) {
            const uint4 d = philox4x32_10(counter, a.seed);
            swap = u01(d.y) < p_swap;
            trow += (long long)int_below(d.x, (uint32_t)K) * (2 * a.C + 6);
        }
    }

    // every load of the table comes before the first store of the kernel (scalar loads)
    AugX ax;
    int ax0 = 0, ax1 = 1, ax2 = 2;
    float sg0 = 1.f, sg1 = 1.f, sg2 = 1.f;
    if (swap && w.is_y) {
        // the binding validates the table; an axis outside 0..2 still reads nothing outside its own triple
        const int32_t* __restrict__ la = trow + 2 * a.C;
        ax0 = (uint32_t)la[0] < 3u ? la[0] : 0, ax1 = (uint32_t)la[1] < 3u ? la[1] : 1, ax2 = (uint32_t)la[2] < 3u ? la[2] : 2;
        sg0 = (float)la[3], sg1 = (float)la[4], sg2 = (float)la[5];
    } else if (swap) {
        ax.map = load_channel_map(trow, a.C);
    }

    if (!w.valid || (w.is_y && !swap)) {        // zero-fill, or targets that no transform touches
        plain_row(w);
        return;
    }

    if (w.is_y) {                               // location (s, axis) <- sign[axis] * location (s, axis[axis]); activity copied
        const uint32_t n_sed = (uint32_t)a.n_sed, cols = 4u * n_sed;
        for (uint64_t off = first_off; off < row; off += tile_step) {
            const uint32_t left = row - (uint32_t)off, len = left < TILE_FLOATS ? left : TILE_FLOATS;
            for (uint32_t i = tid; i < len; i += TILE_THREADS) {
                const uint32_t o = (uint32_t)off + i, j = o % cols;
                float v;
                if (j < n_sed) {
                    v = src[o];
                } else {
                    const uint32_t axis = (j - n_sed) % 3u;
                    const int from = axis == 0u ? ax0 : axis == 1u ? ax1 : ax2;
                    const float sg = axis == 0u ? sg0 : axis == 1u ? sg1 : sg2;
                    v = sg * src[o - axis + (uint32_t)from];
                }
                dst[o] = v;
            }
        }
        return;
    }

    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.F = (uint32_t)a.F;
    ax.T = (uint32_t)a.T;
    ax.FT = ax.F * ax.T;
    ax.fill = a.fill;
    for (uint64_t off = first_off; off < row; off += tile_step) {
        const uint32_t left = row - (uint32_t)off, len = left < TILE_FLOATS ? left : TILE_FLOATS;
        if (a.vec) {
            aug_x_tile_vec(src, dst, (uint32_t)off, (int)len, ax);
        } else {
            for (uint32_t i = tid; i < len; i += TILE_THREADS) dst[(uint32_t)off + i] = aug_x_element(src, (uint32_t)off + i, ax);
        }
    }
}

// ---- gathers with a rotation of the sound field ---------------------------------------------------------------------------
// Channels come in two kinds: the members of a SET that R mixes, and the others, which pass.  A set is a triple
// (cx, cy, cz), the three components of one intensity vector (gather_rows_rot_kernel), or a group of six
// (mx, my, mz, px, py, pz), magnitude and phase of the three directional channels of one microphone
// (gather_rows_polar_kernel).  A predictor row is cut into ITEMS of 16 bytes (4 bytes on the scalar path): a set item is the
// same piece of every channel of its set, loaded, mixed and stored as three or six accesses; a pass item is one piece of
// one channel.  Set items are numbered first, in tiles of their kind (Triples, Groups below), pass items behind them in
// tiles of ROT_TILE_B (four per lane, as the other gathers), so whether a tile mixes is uniform over the workgroup.  A
// sample that draws no rotation has pass items only: it moves as bits.
constexpr int ROT_MAX_TRIPLES = 5, POLAR_MAX_GROUPS = 2;
constexpr int ROT_VEC_A = 2, ROT_VEC_B = TILE_VEC, POLAR_VEC = 1;
constexpr uint32_t ROT_TILE_A = TILE_THREADS * ROT_VEC_A, ROT_TILE_B = TILE_THREADS * ROT_VEC_B,
                   POLAR_TILE = TILE_THREADS * POLAR_VEC;              // items per tile

struct RotParams {
    int n_sets, n_pass;
    uint64_t sets;              // 4 bits per entry: the channels of set 0, of set 1, ...
    uint64_t pass;              // 4 bits per entry: the channels outside the sets, ascending
    float p_rot;
    int mirror, zflip;
};

struct RotX {
    float r[9];                 // row-major
    MaskPair fm, tm;
    uint32_t T, FT, P;          // P: items per channel
    float fill;
};

struct PolarStats {
    float mean_m, sd_m, mean_p, sd_p;
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

// item i of n (set items or pass items): piece i % P of unit i / P (a set, or an entry of `pass`); a lane past the end
// looks at item 0 and neither loads nor stores
struct RotItem {
    uint32_t u, e, t0;          // the unit, the offset of the piece inside a channel, its first frame
    bool whole, live;           // the frequency row is masked; i < n
};
template <bool VEC> __device__ __forceinline__ RotItem rot_item(uint32_t first, int k, uint32_t n, const RotX& a) {
    const uint32_t i = first + threadIdx.x + (uint32_t)k * TILE_THREADS, ii = i < n ? i : 0u;
    RotItem it;
    it.u = ii / a.P;
    it.e = (ii - it.u * a.P) * (VEC ? 4u : 1u);
    const uint32_t f = it.e / a.T;
    it.t0 = it.e - f * a.T;
    it.whole = a.fm.hit(f);
    it.live = i < n;
    return it;
}

// The two kinds of tile that mix: items [first, first + TILE) of the n set items.

// channel triples: two items per lane, six 16-byte loads in flight
struct Triples {
    static constexpr uint32_t TILE = ROT_TILE_A;
    template <bool VEC, bool STATS>
    static __device__ __forceinline__ void tile(const float* __restrict__ s, float* __restrict__ d, uint32_t first, uint32_t n,
                                                uint64_t triples, const RotX& a, const PolarStats&) {
        float4 vx[ROT_VEC_A], vy[ROT_VEC_A], vz[ROT_VEC_A];
        uint32_t ox[ROT_VEC_A], oy[ROT_VEC_A], oz[ROT_VEC_A];
        RotItem it[ROT_VEC_A];
#pragma unroll
        for (int k = 0; k < ROT_VEC_A; ++k) {
            it[k] = rot_item<VEC>(first, k, n, a);
            const uint32_t m = (uint32_t)(triples >> (12u * it[k].u));
            ox[k] = (m & 15u) * a.FT + it[k].e, oy[k] = ((m >> 4) & 15u) * a.FT + it[k].e, oz[k] = ((m >> 8) & 15u) * a.FT + it[k].e;
            const bool load = it[k].live && !it[k].whole;
            const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
            vx[k] = load ? rot_load<VEC>(s + ox[k]) : none;
            vy[k] = load ? rot_load<VEC>(s + oy[k]) : none;
            vz[k] = load ? rot_load<VEC>(s + oz[k]) : none;
        }
#pragma unroll
        for (int k = 0; k < ROT_VEC_A; ++k) {
            if (!it[k].live) continue;
            rot_store<VEC>(d + ox[k], rot_masked(rot_mix4(a.r, vx[k], vy[k], vz[k]), it[k].whole, it[k].t0, a));
            rot_store<VEC>(d + oy[k], rot_masked(rot_mix4(a.r + 3, vx[k], vy[k], vz[k]), it[k].whole, it[k].t0, a));
            rot_store<VEC>(d + oz[k], rot_masked(rot_mix4(a.r + 6, vx[k], vy[k], vz[k]), it[k].whole, it[k].t0, a));
        }
    }
};

// Magnitude / phase groups.  A bin of the STFT is the complex number m e^(i phi) and the STFT is linear, so the rotation is
// the real matrix R applied to the complex 3-vector of every (f, t): polar to Cartesian, mix, back.  With `stats` the
// stored values are standardised, (value - mean) / sd per kind, and the kernel undoes and redoes that around the rotation.
// One (f, t) of one group, in place: m[j], ph[j] (j = x, y, z) as stored -> as stored after the rotation
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

// one item per lane: six 16-byte loads in flight ahead of six stores
struct Groups {
    static constexpr uint32_t TILE = POLAR_TILE;
    template <bool VEC, bool STATS>
    static __device__ __forceinline__ void tile(const float* __restrict__ s, float* __restrict__ d, uint32_t first, uint32_t n,
                                                uint64_t groups, const RotX& a, const PolarStats& st) {
        float4 v[POLAR_VEC][6];
        uint32_t o[POLAR_VEC][6];
        RotItem it[POLAR_VEC];
#pragma unroll
        for (int k = 0; k < POLAR_VEC; ++k) {
            it[k] = rot_item<VEC>(first, k, n, a);
            const uint32_t g = (uint32_t)(groups >> (24u * it[k].u));
            const bool load = it[k].live && !it[k].whole;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                o[k][j] = ((g >> (4 * j)) & 15u) * a.FT + it[k].e;
                v[k][j] = load ? rot_load<VEC>(s + o[k][j]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int k = 0; k < POLAR_VEC; ++k) {
            if (!it[k].live) continue;
            float* lane[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) lane[j] = reinterpret_cast<float*>(&v[k][j]);
#pragma unroll
            for (int q = 0; q < (VEC ? 4 : 1); ++q) {
                float m[3] = {lane[0][q], lane[1][q], lane[2][q]}, ph[3] = {lane[3][q], lane[4][q], lane[5][q]};
                polar_mix<STATS>(a.r, st, m, ph);
#pragma unroll
                for (int j = 0; j < 3; ++j) lane[j][q] = m[j], lane[3 + j][q] = ph[j];
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) rot_store<VEC>(d + o[k][j], rot_masked(v[k][j], it[k].whole, it[k].t0, a));
        }
    }
};

// items [first, first + ROT_TILE_B) of the n pass items: item i is piece i % P of the channel in entry i / P of `pass`
template <bool VEC> __device__ __forceinline__ void rot_tile_pass(const float* __restrict__ s, float* __restrict__ d, uint32_t first,
                                                                  uint32_t n, uint64_t pass, const RotX& a) {
    float4 v[ROT_VEC_B];
    uint32_t o[ROT_VEC_B];
    RotItem it[ROT_VEC_B];
#pragma unroll
    for (int k = 0; k < ROT_VEC_B; ++k) {
        it[k] = rot_item<VEC>(first, k, n, a);
        o[k] = ((uint32_t)(pass >> (4u * it[k].u)) & 15u) * a.FT + it[k].e;
        v[k] = (it[k].live && !it[k].whole) ? rot_load<VEC>(s + o[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < ROT_VEC_B; ++k) {
        if (!it[k].live) continue;
        rot_store<VEC>(d + o[k], rot_masked(v[k], it[k].whole, it[k].t0, a));
    }
}

// the predictor row of one sample: tiles [first, ...) in steps of `step`, the tiles of the sets before the pass tiles
template <class Kind, bool VEC, bool STATS>
__device__ __forceinline__ void rot_x_row(const float* __restrict__ s, float* __restrict__ d, uint32_t first, uint32_t step, uint32_t n_a,
                                          uint32_t n_b, uint64_t sets, uint64_t pass, const RotX& a, const PolarStats& st) {
    const uint32_t tiles_a = (n_a + Kind::TILE - 1u) / Kind::TILE, tiles_b = (n_b + ROT_TILE_B - 1u) / ROT_TILE_B;
    for (uint32_t tile = first; tile < tiles_a + tiles_b; tile += step) {
        if (tile < tiles_a) Kind::template tile<VEC, STATS>(s, d, tile * Kind::TILE, n_a, sets, a, st);
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
        counter = sample_counter(epoch, p);
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
    const uint64_t tile_step = (uint64_t)step * (uint64_t)TILE_FLOATS;
    for (uint64_t off = (uint64_t)first * (uint64_t)TILE_FLOATS; off < row; off += tile_step) {
        const uint32_t left = row - (uint32_t)off, len = left < TILE_FLOATS ? left : TILE_FLOATS;
        for (uint32_t i = threadIdx.x; i < len; i += TILE_THREADS) {
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

// The body of both rotating kernels after the preamble.  Everything up to the tile loops is uniform over the workgroup:
// the draws, the nine entries of R (computed, or loaded from `matrices`), the four statistics (one load; nullptr where
// the Kind has none), the mask bounds.  `epoch`, `matrices` and `stats` are __restrict__ arguments of the kernels and
// are read before the first store: scalar loads.
template <class Kind>
__device__ __forceinline__ void rot_gather(const GatherRow& w, const int32_t* __restrict__ epoch, const float* __restrict__ matrices,
                                           const float* __restrict__ stats, const AugParams& a, const RotParams& q) {
    float* __restrict__ dst = w.dst;
    const float* __restrict__ src = w.src;

    // the draws of this sample; an explicit matrix takes their place
    uint64_t counter = 0;
    RotX ax;
    const bool rotate = rot_draw(w.valid, w.p, blockIdx.y, epoch, matrices, a.seed, q.p_rot, q.mirror, q.zflip, counter, ax);
    PolarStats st{0.f, 1.f, 0.f, 1.f};
    if (stats && rotate && !w.is_y) st = PolarStats{stats[0], stats[1], stats[2], stats[3]};

    if (!w.valid || (w.is_y && !rotate)) {      // zero-fill, or targets that no rotation touches
        plain_row(w);
        return;
    }

    if (w.is_y) {
        rot_y_row(src, dst, (uint32_t)w.row, (uint32_t)w.first, (uint32_t)w.step, (uint32_t)a.n_sed, ax);   // rows are below 2^31 floats
        return;
    }

    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.T = (uint32_t)a.T;
    ax.FT = (uint32_t)a.F * ax.T;
    ax.P = a.vec ? ax.FT >> 2 : ax.FT;
    ax.fill = a.fill;
    const uint32_t first = (uint32_t)w.first, step = (uint32_t)w.step;
    const uint32_t n_a = rotate ? (uint32_t)q.n_sets * ax.P : 0u;
    const uint32_t n_b = (uint32_t)(rotate ? q.n_pass : a.C) * ax.P;
    const uint64_t pass = rotate ? q.pass : 0xFEDCBA9876543210ull;
    if (stats) {
        if (a.vec) rot_x_row<Kind, true, true>(src, dst, first, step, n_a, n_b, q.sets, pass, ax, st);
        else rot_x_row<Kind, false, true>(src, dst, first, step, n_a, n_b, q.sets, pass, ax, st);
    } else {
        if (a.vec) rot_x_row<Kind, true, false>(src, dst, first, step, n_a, n_b, q.sets, pass, ax, st);
        else rot_x_row<Kind, false, false>(src, dst, first, step, n_a, n_b, q.sets, pass, ax, st);
    }
}

// grid (gx + gy, count); 8 waves per SIMD as the other gathers
__global__ __launch_bounds__(TILE_THREADS, 8) void gather_rows_rot_kernel(GatherSide x, GatherSide y, int gx,
                                                                       const int64_t* __restrict__ index, long long n_index,
                                                                       long long n_rows, const int32_t* __restrict__ cursor,
                                                                       long long stride, long long start,
                                                                       const int32_t* __restrict__ epoch,
                                                                       const float* __restrict__ matrices, AugParams a, RotParams q) {
    rot_gather<Triples>(resolve_row(x, y, gx, index, n_index, n_rows, cursor, stride, start), epoch, matrices, nullptr, a, q);
}

// grid (gx + gy, count).  sincosf (with its large-argument reduction) and atan2f, inlined three times each per position,
// fill the registers: 108 VGPRs on gfx950, so the kernel is bounded to 4 waves per SIMD (under the 8 of the other gathers
// it spills); a second item per lane would add 48 registers of data and drop to 3.
__global__ __launch_bounds__(TILE_THREADS, 4) void gather_rows_polar_kernel(GatherSide x, GatherSide y, int gx,
                                                                         const int64_t* __restrict__ index, long long n_index,
                                                                         long long n_rows, const int32_t* __restrict__ cursor,
                                                                         long long stride, long long start,
                                                                         const int32_t* __restrict__ epoch,
                                                                         const float* __restrict__ matrices,
                                                                         const float* __restrict__ stats, AugParams a, RotParams q) {
    rot_gather<Groups>(resolve_row(x, y, gx, index, n_index, n_rows, cursor, stride, start), epoch, matrices, stats, a, q);
}

// ---- gather that mixes two clips ---------------------------------------------------------------------------------------------
// Magnitude and phase of a bin are one complex number and the STFT is linear: the mixture a + g b of two recordings has
// the spectrum z_A + g z_B bin by bin.  The channels are PAIRS (magnitude c, phase c + C / 2), every one of them mixed (W
// is a pair like any other), so a mixed sample has pair items only and an unmixed one pass items only: it moves as bits.
// A pair item is the same piece of both channels of a pair from BOTH rows: four loads in flight ahead of two stores.
constexpr int MIX_VEC = 1, MIX_MAX_CLASSES = 64, MIX_MAX_OVERLAPS = 8;
constexpr uint32_t MIX_TILE = TILE_THREADS * MIX_VEC;
constexpr uint64_t MIX_KEY = 0x9E3779B97F4A7C15ull;         // the four groups of a sample's counter are taken: another key

struct MixParams {
    int overlaps, classes;      // classes: 0 where nothing needs it (no targets and no occupancy table)
    float p_mix, gain_lo, gain_hi;
};

// one (f, t) of one pair, in place: m, ph of row A as stored -> as stored of the mixture with g times (mb, pb) of row B
template <bool STATS> __device__ __forceinline__ void mix_bin(const PolarStats& st, float g, float& m, float& ph, float mb, float pb) {
#pragma clang fp contract(off)
    const float mag_a = STATS ? fmaf(m, st.sd_m, st.mean_m) : m, phi_a = STATS ? fmaf(ph, st.sd_p, st.mean_p) : ph;
    const float mag_b = STATS ? fmaf(mb, st.sd_m, st.mean_m) : mb, phi_b = STATS ? fmaf(pb, st.sd_p, st.mean_p) : pb;
    float sa, ca, sb, cb;
    sincosf(phi_a, &sa, &ca);
    sincosf(phi_b, &sb, &cb);
    const float re = fmaf(g, mag_b * cb, mag_a * ca), im = fmaf(g, mag_b * sb, mag_a * sa);
    const float mag = sqrtf(fmaf(im, im, re * re)), phi = atan2f(im, re);
    m = STATS ? __fdiv_rn(mag - st.mean_m, st.sd_m) : mag;
    ph = STATS ? __fdiv_rn(phi - st.mean_p, st.sd_p) : phi;
}

// items [first, first + MIX_TILE) of the n pair items: item i is piece i % P of pair i / P; `half`: floats between the
// magnitude and the phase channel of a pair
template <bool VEC, bool STATS>
__device__ __forceinline__ void mix_tile(const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ d, uint32_t first,
                                         uint32_t n, uint32_t half, float g, const RotX& a, const PolarStats& st) {
    float4 v[MIX_VEC][4];
    uint32_t om[MIX_VEC];
    RotItem it[MIX_VEC];
#pragma unroll
    for (int k = 0; k < MIX_VEC; ++k) {
        it[k] = rot_item<VEC>(first, k, n, a);
        om[k] = it[k].u * a.FT + it[k].e;
        const bool load = it[k].live && !it[k].whole;           // a masked frequency row is read from neither clip
        const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
        v[k][0] = load ? rot_load<VEC>(sa + om[k]) : none;
        v[k][1] = load ? rot_load<VEC>(sa + om[k] + half) : none;
        v[k][2] = load ? rot_load<VEC>(sb + om[k]) : none;
        v[k][3] = load ? rot_load<VEC>(sb + om[k] + half) : none;
    }
#pragma unroll
    for (int k = 0; k < MIX_VEC; ++k) {
        if (!it[k].live) continue;
        float* lane[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) lane[j] = reinterpret_cast<float*>(&v[k][j]);
#pragma unroll
        for (int q = 0; q < (VEC ? 4 : 1); ++q) mix_bin<STATS>(st, g, lane[0][q], lane[1][q], lane[2][q], lane[3][q]);
        rot_store<VEC>(d + om[k], rot_masked(v[k][0], it[k].whole, it[k].t0, a));
        rot_store<VEC>(d + om[k] + half, rot_masked(v[k][1], it[k].whole, it[k].t0, a));
    }
}

// the predictor row of one sample: n_a pair items (a mixed sample) in tiles of MIX_TILE, then n_b pass items (an unmixed one)
template <bool VEC, bool STATS>
__device__ __forceinline__ void mix_x_row(const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ d, uint32_t first,
                                          uint32_t step, uint32_t n_a, uint32_t n_b, uint32_t half, float g, const RotX& a,
                                          const PolarStats& st) {
    const uint32_t tiles_a = (n_a + MIX_TILE - 1u) / MIX_TILE, tiles_b = (n_b + ROT_TILE_B - 1u) / ROT_TILE_B;
    for (uint32_t tile = first; tile < tiles_a + tiles_b; tile += step) {
        if (tile < tiles_a) mix_tile<VEC, STATS>(sa, sb, d, tile * MIX_TILE, n_a, half, g, a, st);
        else rot_tile_pass<VEC>(sa, d, (tile - tiles_a) * ROT_TILE_B, n_b, 0xFEDCBA9876543210ull, a);
    }
}

// The target row of a mixed sample.  Per (frame, class) the list of A's active slots in slot order, then B's; output slot k
// of the class takes activity and location of entry k as bits, +0 behind the list; entries past `overlaps` are dropped
// (the occupancy test keeps a sample whose clips could overflow from being mixed at all).  Active: activity > 0.5f, so a
// NaN is not.  One writer per element.
__device__ __forceinline__ void mix_y_row(const float* __restrict__ sa, const float* __restrict__ sb, float* __restrict__ dst, uint32_t row,
                                          uint32_t first, uint32_t step, uint32_t n_sed, uint32_t overlaps) {
    const uint32_t cols = 4u * n_sed;
    const uint64_t tile_step = (uint64_t)step * (uint64_t)TILE_FLOATS;
    for (uint64_t off = (uint64_t)first * (uint64_t)TILE_FLOATS; off < row; off += tile_step) {
        const uint32_t left = row - (uint32_t)off, len = left < TILE_FLOATS ? left : TILE_FLOATS;
        for (uint32_t i = threadIdx.x; i < len; i += TILE_THREADS) {
            const uint32_t o = (uint32_t)off + i, j = o % cols, base = o - j;
            const bool act = j < n_sed;
            const uint32_t s = act ? j : (j - n_sed) / 3u, axis = act ? 0u : (j - n_sed) - 3u * s;
            const uint32_t c0 = s - s % overlaps, k = s - c0;       // the first slot of the class, the place in it
            uint32_t seen = 0u, pick = 2u * overlaps;
            for (uint32_t e = 0u; e < 2u * overlaps; ++e) {
                const float v = e < overlaps ? sa[base + c0 + e] : sb[base + c0 + e - overlaps];
                if (v > 0.5f) {
                    if (seen == k) pick = e;
                    ++seen;
                }
            }
            float out = 0.f;
            if (pick < 2u * overlaps) {
                const float* __restrict__ src = pick < overlaps ? sa : sb;
                const uint32_t from = c0 + (pick < overlaps ? pick : pick - overlaps);
                out = src[base + (act ? from : n_sed + 3u * from + axis)];
            }
            dst[o] = out;
        }
    }
}

// grid (gx + gy, count).  Everything up to the tile loops is uniform over the workgroup: the draw or the explicit partner
// and gain, the partner's resident row, the 2 * classes bytes of the occupancy test, the four statistics, the mask bounds.
// `epoch`, `partners`, `gains`, `stats` and `occupancy` are __restrict__ arguments and are read before the first store.
// Two sincosf and one atan2f per position: 74 VGPRs on gfx950, 6 waves per SIMD (gather_rows_polar_kernel, with three of
// each, has 108 and 4); under the 8 of the plain gathers it would spill.
__global__ __launch_bounds__(TILE_THREADS, 6) void gather_rows_mix_kernel(GatherSide x, GatherSide y, int gx,
                                                                       const int64_t* __restrict__ index, long long n_index,
                                                                       long long n_rows, const int32_t* __restrict__ cursor,
                                                                       long long stride, long long start,
                                                                       const int32_t* __restrict__ epoch,
                                                                       const int64_t* __restrict__ partners,
                                                                       const float* __restrict__ gains, const float* __restrict__ stats,
                                                                       const uint8_t* __restrict__ occupancy, AugParams a, MixParams q) {
    const GatherRow w = resolve_row(x, y, gx, index, n_index, n_rows, cursor, stride, start);

    // the partner of this sample and its gain: explicit, or drawn with the key of the mix
    uint64_t counter = 0;
    long long r2 = -1;
    float g = 0.f;
    if (w.valid) {
        counter = sample_counter(epoch, w.p);
        long long p2 = -1;
        if (partners) {
            p2 = partners[blockIdx.y];
            g = gains[blockIdx.y];
        } else if (q.p_mix > 0.f && n_index > 1) {
            const uint4 d = philox4x32_10(counter, a.seed ^ MIX_KEY);
            if (u01(d.y) < q.p_mix) {           // (p + 1 + int(w[0], n_index - 1)) mod n_index: the sum is below 2 * n_index
                p2 = w.p + 1 + (long long)int_below(d.x, (uint32_t)(n_index - 1));
                if (p2 >= n_index) p2 -= n_index;
            }
            g = fmaf(u01(d.z), q.gain_hi - q.gain_lo, q.gain_lo);
        }
        if (p2 >= 0 && p2 < n_index) r2 = index[p2];
        if (r2 >= n_rows) r2 = -1;
    }
    bool mix = r2 >= 0;
    if (mix && occupancy) {                     // no class may hold more events in the two clips than it has slots
        const uint8_t* __restrict__ oa = occupancy + w.r * q.classes;
        const uint8_t* __restrict__ ob = occupancy + r2 * q.classes;
        for (int c = 0; c < q.classes; ++c) mix &= (int)oa[c] + (int)ob[c] <= q.overlaps;
    }
    PolarStats st{0.f, 1.f, 0.f, 1.f};
    if (stats && mix && !w.is_y) st = PolarStats{stats[0], stats[1], stats[2], stats[3]};

    if (!w.valid || (w.is_y && !mix)) {         // zero-fill, or targets of a sample that is not mixed
        plain_row(w);
        return;
    }

    const GatherSide sd = w.is_y ? y : x;
    const float* __restrict__ src = w.src;
    const float* __restrict__ src2 = mix ? sd.all + r2 * sd.row : w.src;
    float* __restrict__ dst = w.dst;
    const uint32_t first = (uint32_t)w.first, step = (uint32_t)w.step;
    if (w.is_y) {
        mix_y_row(src, src2, dst, (uint32_t)w.row, first, step, (uint32_t)a.n_sed, (uint32_t)q.overlaps);     // rows are below 2^31 floats
        return;
    }

    RotX ax;
    ax.fm = draw_masks(counter | 1u, a.seed, a.n_fmask, a.f_max, a.F);
    ax.tm = draw_masks(counter | 2u, a.seed, a.n_tmask, a.t_max, a.T);
    ax.T = (uint32_t)a.T;
    ax.FT = (uint32_t)a.F * ax.T;
    ax.P = a.vec ? ax.FT >> 2 : ax.FT;
    ax.fill = a.fill;
    const uint32_t pairs = (uint32_t)a.C >> 1, n_a = mix ? pairs * ax.P : 0u, n_b = mix ? 0u : (uint32_t)a.C * ax.P;
    const uint32_t half = pairs * ax.FT;
    if (stats) {
        if (a.vec) mix_x_row<true, true>(src, src2, dst, first, step, n_a, n_b, half, g, ax, st);
        else mix_x_row<false, true>(src, src2, dst, first, step, n_a, n_b, half, g, ax, st);
    } else {
        if (a.vec) mix_x_row<true, false>(src, src2, dst, first, step, n_a, n_b, half, g, ax, st);
        else mix_x_row<false, false>(src, src2, dst, first, step, n_a, n_b, half, g, ax, st);
    }
}

// occ[r, c]: the largest number of active slots of class c in one frame of target row r.  A workgroup per row (and
// onwards in steps of the grid), a lane per class: neighbouring lanes read neighbouring slots.  One writer per byte.
__global__ __launch_bounds__(MIX_MAX_CLASSES) void target_occupancy_kernel(const float* __restrict__ y_all, long long n_rows,
                                                                          uint32_t row_y, uint32_t cols, uint32_t overlaps,
                                                                          uint32_t classes, uint8_t* __restrict__ occ) {
    const uint32_t c = threadIdx.x;
    if (c >= classes) return;
    for (long long r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const float* __restrict__ src = y_all + r * (long long)row_y;
        uint32_t most = 0u;
        for (uint32_t base = 0u; base < row_y; base += cols) {
            uint32_t n = 0u;
            for (uint32_t e = 0u; e < overlaps; ++e) n += src[base + c * overlaps + e] > 0.5f ? 1u : 0u;
            most = n > most ? n : most;
        }
        occ[r * classes + c] = (uint8_t)most;
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

// ---- host side ------------------------------------------------------------------------------------------------------------
// the arguments every gather takes, in the order of the C ABI
struct GatherArgs {
    const float* x_all;
    int64_t row_x;
    float* out_x;
    const float* y_all;
    int64_t row_y;
    float* out_y;
    const int64_t* index;
    int64_t n_index, n_rows;
    const int32_t* cursor;
    int64_t cursor_stride, start;
    int32_t B, count;
    bool has_x() const { return x_all || out_x; }
    bool has_y() const { return y_all || out_y; }
};

// what all four entry points refuse (SELD_EINVAL)
static bool gather_refused(const GatherArgs& g) {
    if (!g.index || g.n_index <= 0 || g.n_rows <= 0 || g.B <= 0 || g.count <= 0 || g.count > g.B || g.count > 65535) return true;
    if (!g.has_x() && !g.has_y()) return true;
    if (g.has_x() && (!g.x_all || !g.out_x || g.row_x <= 0)) return true;
    if (g.has_y() && (!g.y_all || !g.out_y || g.row_y <= 0)) return true;
    return g.cursor && g.cursor_stride < 0;
}

// on top of it, what the augmenting entry points refuse (SELD_EINVAL) of the arguments they share
static bool aug_gather_refused(const GatherArgs& g, const AugParams& a, int32_t y_cols, const int32_t* epoch) {
    if (gather_refused(g) || g.n_index > (1ll << 32)) return true;
    if (!epoch || a.C < 1 || a.C > MAP_MAX_C || a.F < 1 || a.T < 1) return true;
    if (a.n_fmask < 0 || a.n_fmask > 2 || a.n_tmask < 0 || a.n_tmask > 2 || a.f_max < 0 || a.f_max > a.F || a.t_max < 0 || a.t_max > a.T)
        return true;
    if (g.has_x() && (long long)a.C * a.F * a.T != g.row_x) return true;            // 16 * 2^31 * 2^31 fits an int64
    return g.has_y() && (y_cols < 4 || y_cols % 4 || g.row_y % y_cols);
}

// and what they do not support: offsets inside a row are 32-bit
static bool long_rows(const GatherArgs& g) { return g.row_x >= (1ll << 31) || g.row_y >= (1ll << 31); }

// the shared members of the augmenting kernels' parameters
static AugParams aug_params(const GatherArgs& g, int32_t C, int32_t F, int32_t T, int32_t y_cols, uint64_t seed, int32_t n_fmask,
                            int32_t f_max, int32_t n_tmask, int32_t t_max, float fill) {
    const int vec = g.has_x() && T % 4 == 0 && (((uintptr_t)g.x_all | (uintptr_t)g.out_x) & 15) == 0;
    return AugParams{C, F, T, g.has_y() && y_cols >= 4 ? y_cols / 4 : 0, seed, n_fmask, f_max, n_tmask, t_max, fill, vec};
}

static long long tiles_of(long long items, long long tile) { return (items + tile - 1) / tile; }

// The launch plan of every gather: a predictor row of `tiles_x` tiles and a target row of row_y floats over the grid
// (gx + gy, count), each side capped so that the grid stays near TILE_MAX_BLOCKS workgroups.  `tail`: what the kernel
// takes behind the arguments all of them share.
template <class Kernel, class... Tail>
static int launch_gather(Kernel kernel, const GatherArgs& g, long long tiles_x, void* stream, Tail... tail) {
    const long long cap = TILE_MAX_BLOCKS / g.count > 0 ? TILE_MAX_BLOCKS / g.count : 1;
    const long long tx = g.has_x() ? tiles_x : 0, ty = g.has_y() ? tiles_of(g.row_y, TILE_FLOATS) : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{g.x_all, g.out_x, g.has_x() ? (long long)g.row_x : 0}, y{g.y_all, g.out_y, g.has_y() ? (long long)g.row_y : 0};
    hipLaunchKernelGGL(kernel, dim3(gx + gy, g.count), dim3(TILE_THREADS), 0, (hipStream_t)stream, x, y, gx, g.index, (long long)g.n_index,
                       (long long)g.n_rows, g.cursor, (long long)g.cursor_stride, (long long)g.start, tail...);
    return check_launch();
}

extern "C" int seld_gather_rows(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                int64_t cursor_stride, int64_t start, int32_t B, int32_t count, void* stream) {
    const GatherArgs g{x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, start, B, count};
    if (gather_refused(g)) return SELD_EINVAL;
    return launch_gather(gather_rows_kernel, g, tiles_of(row_x, TILE_FLOATS), stream);
}

extern "C" int seld_gather_rows_aug(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                    float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                    int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                    int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, const int32_t* table,
                                    int32_t K, float p_swap, int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max,
                                    float fill, void* stream) {
    const GatherArgs g{x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, start, B, count};
    const AugParams a = aug_params(g, C, F, T, y_cols, seed, n_fmask, f_max, n_tmask, t_max, fill);
    if (aug_gather_refused(g, a, y_cols, epoch)) return SELD_EINVAL;
    if (K < 0 || K > MAP_MAX_K || (K > 0) != (table != nullptr)) return SELD_EINVAL;
    if (!(p_swap >= 0.f && p_swap <= 1.f)) return SELD_EINVAL;                      // a NaN fails both
    if (long_rows(g)) return SELD_EUNSUPPORTED;
    return launch_gather(gather_rows_aug_kernel, g, tiles_of(row_x, TILE_FLOATS), stream, epoch, table, a, (int)K, p_swap);
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

// What the two rotating entry points do alike, from the check of their sets on: `n_sets` sets (at most `max_sets`) of
// `width` channels each, mixed in tiles of `tile` items.  The sets travel by value, so their content is checked here: the
// kernel then indexes with them as they are.  The grid covers the larger of a rotated and an unrotated sample's tiling.
template <class Kernel, class... Stats>
static int launch_rotating(Kernel kernel, const GatherArgs& g, const AugParams& a, int32_t y_cols, const int32_t* epoch, uint64_t sets,
                           int32_t n_sets, int max_sets, int width, uint32_t tile, float p_rot, int32_t mirror, int32_t zflip,
                           const float* matrices, void* stream, Stats... stats) {
    if (aug_gather_refused(g, a, y_cols, epoch)) return SELD_EINVAL;
    if (n_sets < 1 || n_sets > max_sets || width * n_sets > a.C) return SELD_EINVAL;
    if (!(p_rot >= 0.f && p_rot <= 1.f)) return SELD_EINVAL;                        // a NaN fails both
    if (long_rows(g)) return SELD_EUNSUPPORTED;
    RotParams q{n_sets, 0, sets, 0, p_rot, mirror != 0, zflip != 0};
    if (packed_channels_refused(sets, width * n_sets, a.C, q.pass, q.n_pass)) return SELD_EINVAL;      // at most 60 bits are entries
    const long long P = a.vec ? (long long)a.F * a.T / 4 : (long long)a.F * a.T;
    const long long t_rot = tiles_of(n_sets * P, tile) + tiles_of(q.n_pass * P, ROT_TILE_B), t_plain = tiles_of(a.C * P, ROT_TILE_B);
    return launch_gather(kernel, g, t_rot > t_plain ? t_rot : t_plain, stream, epoch, matrices, stats..., a, q);
}

extern "C" int seld_gather_rows_rot(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                    float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                    int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                    int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, uint64_t triples,
                                    int32_t n_triples, float p_rot, int32_t rot_mirror, int32_t rot_zflip, const float* matrices,
                                    int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max, float fill, void* stream) {
    const GatherArgs g{x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, start, B, count};
    const AugParams a = aug_params(g, C, F, T, y_cols, seed, n_fmask, f_max, n_tmask, t_max, fill);
    return launch_rotating(gather_rows_rot_kernel, g, a, y_cols, epoch, triples, n_triples, ROT_MAX_TRIPLES, 3, ROT_TILE_A, p_rot,
                           rot_mirror, rot_zflip, matrices, stream);
}

extern "C" int seld_gather_rows_polar(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                      float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                      int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                      int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, uint64_t groups,
                                      int32_t n_groups, const float* stats, float p_rot, int32_t rot_mirror, int32_t rot_zflip,
                                      const float* matrices, int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max,
                                      float fill, void* stream) {
    const GatherArgs g{x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, start, B, count};
    const AugParams a = aug_params(g, C, F, T, y_cols, seed, n_fmask, f_max, n_tmask, t_max, fill);
    return launch_rotating(gather_rows_polar_kernel, g, a, y_cols, epoch, groups, n_groups, POLAR_MAX_GROUPS, 6, POLAR_TILE, p_rot,
                           rot_mirror, rot_zflip, matrices, stream, stats);
}

extern "C" int seld_target_occupancy(const float* y_all, int64_t n_rows, int64_t row_y, int32_t y_cols, int32_t overlaps, uint8_t* occ,
                                     void* stream) {
    if (!y_all || !occ || n_rows <= 0 || row_y <= 0 || y_cols <= 0 || overlaps <= 0) return SELD_EINVAL;
    if (y_cols % (4ll * overlaps) || row_y % y_cols) return SELD_EINVAL;
    const int classes = y_cols / (4 * overlaps);
    if (classes > MIX_MAX_CLASSES || overlaps > MIX_MAX_OVERLAPS || row_y >= (1ll << 31)) return SELD_EUNSUPPORTED;
    const long long cap = 1ll << 16;
    hipLaunchKernelGGL(target_occupancy_kernel, dim3((unsigned)(n_rows < cap ? n_rows : cap)), dim3(MIX_MAX_CLASSES), 0, (hipStream_t)stream,
                       y_all, (long long)n_rows, (uint32_t)row_y, (uint32_t)y_cols, (uint32_t)overlaps, (uint32_t)classes, occ);
    return check_launch();
}

// The grid covers the larger of a mixed and an unmixed sample's tiling, as that of the rotating gathers.
extern "C" int seld_gather_rows_mix(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                    float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                    int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F,
                                    int32_t T, int32_t y_cols, const int32_t* epoch, uint64_t seed, int32_t overlaps,
                                    const float* stats, float p_mix, float gain_lo, float gain_hi, const int64_t* partners,
                                    const float* gains, const uint8_t* occupancy, int32_t n_fmask, int32_t f_max, int32_t n_tmask,
                                    int32_t t_max, float fill, void* stream) {
    const GatherArgs g{x_all, row_x, out_x, y_all, row_y, out_y, index, n_index, n_rows, cursor, cursor_stride, start, B, count};
    const AugParams a = aug_params(g, C, F, T, y_cols, seed, n_fmask, f_max, n_tmask, t_max, fill);
    if (aug_gather_refused(g, a, y_cols, epoch)) return SELD_EINVAL;
    if (C % 2 || overlaps < 1) return SELD_EINVAL;
    const bool slots = g.has_y() || occupancy;                                      // what reads y_cols as classes * overlaps
    if (slots && (y_cols < 4 || y_cols % (4ll * overlaps))) return SELD_EINVAL;
    if (!(p_mix >= 0.f && p_mix <= 1.f)) return SELD_EINVAL;                        // a NaN fails both
    if (!(gain_lo > 0.f && gain_lo <= gain_hi && gain_hi < INFINITY)) return SELD_EINVAL;
    if ((partners != nullptr) != (gains != nullptr)) return SELD_EINVAL;
    const int classes = slots ? y_cols / (4 * overlaps) : 0;
    if (classes > MIX_MAX_CLASSES || overlaps > MIX_MAX_OVERLAPS || long_rows(g)) return SELD_EUNSUPPORTED;
    const MixParams q{overlaps, classes, p_mix, gain_lo, gain_hi};
    const long long P = a.vec ? (long long)a.F * a.T / 4 : (long long)a.F * a.T;
    const long long t_mix = tiles_of(a.C / 2 * P, MIX_TILE), t_plain = tiles_of(a.C * P, ROT_TILE_B);
    return launch_gather(gather_rows_mix_kernel, g, t_mix > t_plain ? t_mix : t_plain, stream, epoch, partners, gains, stats, occupancy, a, q);
}

extern "C" int seld_epoch_step_end(const float* loss, float* mean, int32_t* cursor, void* stream) {
    if (!loss || !mean || !cursor) return SELD_EINVAL;
    hipLaunchKernelGGL(epoch_step_end_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, mean, cursor);
    return check_launch();
}
