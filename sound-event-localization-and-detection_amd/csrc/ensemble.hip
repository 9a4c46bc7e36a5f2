// Whole-recording inference: from resident recordings to one (frames, classes * overlaps) track per recording.
//
//   seld_window_batch      one batch of model inputs cut out of the recordings, each under one row of the FOA transform
//                          table (the members m = (r * S + s) * K + k of the ensemble), in one launch
//   seld_ensemble_combine  the members' outputs stitched back: DOAs mapped back through their row, the slots of a
//                          (frame, class) aligned to an anchor member, a weighted mean over windows and transforms
//
// window_batch moves data as loader.hip's augmented gather does, with another address, and shares its tile geometry, the
// packed channel map of a table row and flipop with it (channel_map.h).  Recording, window and table row depend on
// blockIdx.y alone and stay on the scalar unit.  A lane needs (c, f, j) of its output offset (two unsigned divisions by
// uniform divisors per 16 bytes); with T, hop and L multiples of 4 a float4 lies in one (c, f) row and wholly inside or
// wholly past L.
//
// ensemble_combine is small (config 3 at K = 16: 14 MB of members per recording) and bound by latency and reads: one
// thread per (recording, frame, class) walks the covering members in order, so neighbouring lanes read neighbouring
// slots of one frame and every sum has one writer and one order.  A member's table row is the same for every lane:
// scalar loads.  No LDS, no atomics.
#include "channel_map.h"

namespace seld {

constexpr int ENS_MAX_N = 64;

struct WinParams {
    int C, F, L, T, hop, S, K;
    long long m0;
    int vec;                    // T, hop, L multiples of 4 and both arrays 16-byte aligned
};

// grid (gx, count): workgroup x of a row takes the tiles x, x + gx, ... of output row blockIdx.y
__global__ __launch_bounds__(TILE_THREADS, 8) void window_batch_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                      const int32_t* __restrict__ table, WinParams a) {
    const int tid = threadIdx.x;
    const long long m = a.m0 + blockIdx.y;
    const int K1 = a.K > 0 ? a.K : 1;
    const int k = (int)(m % K1);
    const long long rs = m / K1;
    const int s = (int)(rs % a.S);
    const long long r = rs / a.S;
    const uint32_t F = (uint32_t)a.F, T = (uint32_t)a.T, FL = F * (uint32_t)a.L, L = (uint32_t)a.L;
    const uint32_t row = (uint32_t)a.C * F * T;                         // below 2^31, as C * F * L
    const long long t0 = (long long)s * a.hop;
    const long long room = (long long)a.L - t0;
    const uint32_t live = room <= 0 ? 0u : room < (long long)T ? (uint32_t)room : T;     // j < live <=> t0 + j < L
    const float* __restrict__ src = x + r * ((long long)a.C * a.F * a.L) + (live ? t0 : 0);
    float* __restrict__ dst = out + (long long)blockIdx.y * row;

    // the row of the table before the first store of the kernel: scalar loads
    ChannelMap map;
    if (a.K > 0) map = load_channel_map(table + (long long)k * (2 * a.C + 6), a.C);

    for (uint64_t off = (uint64_t)blockIdx.x * TILE_FLOATS; off < row; off += (uint64_t)gridDim.x * TILE_FLOATS) {
        const uint32_t left = row - (uint32_t)off, len = left < TILE_FLOATS ? left : TILE_FLOATS;
        if (a.vec) {                            // row and off are multiples of 4: so is len
            const int nv = (int)(len >> 2);
            float4 v[TILE_VEC];
            uint32_t flip[TILE_VEC];
#pragma unroll
            for (int i = 0; i < TILE_VEC; ++i) {
                const int e = tid + i * TILE_THREADS;
                const uint32_t o = (uint32_t)off + 4u * (uint32_t)(e < nv ? e : 0);
                const uint32_t q = o / T, j = o - q * T, c = q / F, f = q - c * F;
                const uint32_t sc = map.source(c);
                flip[i] = map.flip_of(c);
                v[i] = (e < nv && j < live) ? *reinterpret_cast<const float4*>(src + (sc * FL + f * L + j))
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < TILE_VEC; ++i) {
                const int e = tid + i * TILE_THREADS;
                if (e >= nv) continue;
                float4 w;
                w.x = flipop(v[i].x, flip[i]);
                w.y = flipop(v[i].y, flip[i]);
                w.z = flipop(v[i].z, flip[i]);
                w.w = flipop(v[i].w, flip[i]);
                *reinterpret_cast<float4*>(dst + (uint32_t)off + 4u * (uint32_t)e) = w;
            }
        } else {
            for (uint32_t i = tid; i < len; i += TILE_THREADS) {
                const uint32_t o = (uint32_t)off + i;
                const uint32_t q = o / T, j = o - q * T, c = q / F, f = q - c * F;
                const uint32_t sc = map.source(c);
                const float v = j < live ? src[sc * FL + f * L + j] : 0.f;
                dst[o] = flipop(v, map.flip_of(c));
            }
        }
    }
}

// ---- combine ---------------------------------------------------------------------------------------------------------
constexpr int COMBINE_THREADS = 64;         // 8400 cells per config-3 recording: small workgroups reach more CUs

struct CombineParams {
    long long R;
    int S, K, T_out, hop_out, frames;
    int cells;                  // cells of a frame: classes with the alignment, classes * overlaps (O = 1) without
    int perm_div;               // cells per entry of perm: 1, or overlaps without the alignment
    int t_span;                 // frames, or with perm max(frames, (S - 1) * hop_out + T_out): the -1 entries have a writer
    int stride;                 // ints in a row of the table, 2 * C + 6
};

__device__ __forceinline__ float ens_pick(int j, float v0, float v1, float v2) { return j == 0 ? v0 : (j == 1 ? v1 : v2); }

// One member's slots of a cell: activity p[o] and the DOA mapped back through the row (inverse axes ia, their signs sg).
template <int O>
struct Slots {
    float p[O], q[O][3];
};
template <int O>
__device__ __forceinline__ Slots<O> load_member(const float* __restrict__ sed, const float* __restrict__ doa, size_t at,
                                                int ia0, int ia1, int ia2, float sg0, float sg1, float sg2) {
#pragma clang fp contract(off)
    Slots<O> m;
#pragma unroll
    for (int o = 0; o < O; ++o) {
        m.p[o] = sed[at + o];
        const float d0 = doa[3 * (at + o)], d1 = doa[3 * (at + o) + 1], d2 = doa[3 * (at + o) + 2];
        m.q[o][0] = sg0 * ens_pick(ia0, d0, d1, d2);
        m.q[o][1] = sg1 * ens_pick(ia1, d0, d1, d2);
        m.q[o][2] = sg2 * ens_pick(ia2, d0, d1, d2);
    }
    return m;
}

// the inverse of a row's label map location'[a] = sign[a] * location[axis[a]]: location[b] = sign[a] * location'[a] with
// axis[a] == b.  The binding validates the table; whatever a row holds, nothing outside it is read.
struct Inverse {
    int ia0, ia1, ia2;
    float sg0, sg1, sg2;
};
__device__ __forceinline__ Inverse row_inverse(const int32_t* __restrict__ table, int k, int stride) {
    Inverse v{0, 1, 2, 1.f, 1.f, 1.f};
    if (table) {
        const int32_t* __restrict__ la = table + (long long)k * stride + (stride - 6);
        const int a0 = (uint32_t)la[0] < 3u ? la[0] : 0, a1 = (uint32_t)la[1] < 3u ? la[1] : 1;    // of a permutation, a2 is the one left
        const float s0 = (float)la[3], s1 = (float)la[4], s2 = (float)la[5];
        v.ia0 = a0 == 0 ? 0 : a1 == 0 ? 1 : 2;
        v.ia1 = a0 == 1 ? 0 : a1 == 1 ? 1 : 2;
        v.ia2 = a0 == 2 ? 0 : a1 == 2 ? 1 : 2;
        v.sg0 = ens_pick(v.ia0, s0, s1, s2);
        v.sg1 = ens_pick(v.ia1, s0, s1, s2);
        v.sg2 = ens_pick(v.ia2, s0, s1, s2);
    }
    return v;
}

#define ENS_TRY2(j0, j1, idx)                                                                                         \
    {                                                                                                                 \
        const float c_ = P[0][j0] + P[1][j1];                                                                         \
        if (c_ < best) { best = c_; bi = idx; s0 = j0; s1 = j1; }                                                     \
    }
#define ENS_TRY3(j0, j1, j2, idx)                                                                                     \
    {                                                                                                                 \
        const float c_ = (P[0][j0] + P[1][j1]) + P[2][j2];                                                            \
        if (c_ < best) { best = c_; bi = idx; s0 = j0; s1 = j1; s2 = j2; }                                            \
    }

// one thread per (r, t, cell); O slots per cell; ALIGN only with O in 2..3
template <int O, bool ALIGN>
__global__ __launch_bounds__(COMBINE_THREADS) void ensemble_combine_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                                           const float* __restrict__ win,
                                                                           const int32_t* __restrict__ table,
                                                                           float* __restrict__ out_sed, float* __restrict__ out_doa,
                                                                           int32_t* __restrict__ perm, CombineParams a) {
#pragma clang fp contract(off)
    const long long id = (long long)blockIdx.x * COMBINE_THREADS + threadIdx.x;
    const long long total = a.R * a.t_span * a.cells;
    if (id >= total) return;
    const int c = (int)(id % a.cells);
    const long long rt = id / a.cells;
    const int t = (int)(rt % a.t_span);
    const long long r = rt / a.t_span;
    const int K1 = a.K > 0 ? a.K : 1;
    const int n = a.cells * O;                                          // classes * overlaps either way
    // covering windows: 0 <= t - s * hop_out < T_out
    const int s_hi = min(a.S - 1, t / a.hop_out);
    const int s_lo = t < a.T_out ? 0 : (t - a.T_out) / a.hop_out + 1;
    const bool writes_perm = perm && c % a.perm_div == 0;
    const int perm_cols = a.cells / a.perm_div, perm_c = c / a.perm_div;

    if (t >= a.frames) {                                                // only with perm: the positions past the recording
        if (writes_perm)
            for (int s = s_lo; s <= s_hi; ++s)
                for (int k = 0; k < K1; ++k)
                    perm[((((size_t)r * a.S + s) * K1 + k) * a.T_out + (t - s * a.hop_out)) * perm_cols + perm_c] = -1;
        return;
    }

    // the anchor: the covering window with the largest weight, the first of equals, under row 0
    Slots<O> A;
    if (ALIGN && s_lo <= s_hi) {
        int sa = s_lo;
        float wa = win[t - s_lo * a.hop_out];
        for (int s = s_lo + 1; s <= s_hi; ++s) {
            const float w = win[t - s * a.hop_out];
            if (w > wa) { wa = w; sa = s; }
        }
        const Inverse iv = row_inverse(table, 0, a.stride);
        const size_t at = ((((size_t)r * a.S + sa) * K1) * a.T_out + (t - sa * a.hop_out)) * n + (size_t)c * O;
        A = load_member<O>(sed, doa, at, iv.ia0, iv.ia1, iv.ia2, iv.sg0, iv.sg1, iv.sg2);
    }

    float acc_p[O], acc_q[O][3], wsum = 0.f;
#pragma unroll
    for (int o = 0; o < O; ++o) acc_p[o] = acc_q[o][0] = acc_q[o][1] = acc_q[o][2] = 0.f;
    for (int s = s_lo; s <= s_hi; ++s) {
        const int j = t - s * a.hop_out;
        const float w = win[j];
        for (int k = 0; k < K1; ++k) {
            const Inverse iv = row_inverse(table, k, a.stride);
            const size_t cell = (((size_t)r * a.S + s) * K1 + k) * a.T_out + j;
            const Slots<O> m = load_member<O>(sed, doa, cell * n + (size_t)c * O, iv.ia0, iv.ia1, iv.ia2, iv.sg0, iv.sg1, iv.sg2);
            int bi = 0, s0 = 0, s1 = 1, s2 = 2;
            if constexpr (ALIGN) {
                float P[O][O];          // P[o][i]: output slot o takes member slot i
#pragma unroll
                for (int o = 0; o < O; ++o)
#pragma unroll
                    for (int i = 0; i < O; ++i) {
                        const float dp = m.p[i] - A.p[o], d0 = m.q[i][0] - A.q[o][0], d1 = m.q[i][1] - A.q[o][1],
                                    d2 = m.q[i][2] - A.q[o][2];
                        P[o][i] = ((dp * dp + d0 * d0) + d1 * d1) + d2 * d2;
                    }
                // lexicographic order, from the identity, replaced on `<` only: ties and NaN costs keep the lower index
                float best;
                if constexpr (O == 2) {
                    best = P[0][0] + P[1][1];
                    ENS_TRY2(1, 0, 1)
                } else {
                    best = (P[0][0] + P[1][1]) + P[2][2];
                    ENS_TRY3(0, 2, 1, 1)
                    ENS_TRY3(1, 0, 2, 2)
                    ENS_TRY3(1, 2, 0, 3)
                    ENS_TRY3(2, 0, 1, 4)
                    ENS_TRY3(2, 1, 0, 5)
                }
            }
            (void)s2;
            wsum += w;
#pragma unroll
            for (int o = 0; o < O; ++o) {
                float vp, v0, v1, v2;
                if constexpr (ALIGN) {
                    constexpr int Z = O - 1;        // the last slot: ens_pick's third operand (O == 2: never picked)
                    const int i = o == 0 ? s0 : (o == 1 ? s1 : s2);
                    vp = ens_pick(i, m.p[0], m.p[1], m.p[Z]);
                    v0 = ens_pick(i, m.q[0][0], m.q[1][0], m.q[Z][0]);
                    v1 = ens_pick(i, m.q[0][1], m.q[1][1], m.q[Z][1]);
                    v2 = ens_pick(i, m.q[0][2], m.q[1][2], m.q[Z][2]);
                } else {
                    vp = m.p[o]; v0 = m.q[o][0]; v1 = m.q[o][1]; v2 = m.q[o][2];
                }
                acc_p[o] += w * vp;
                acc_q[o][0] += w * v0;
                acc_q[o][1] += w * v1;
                acc_q[o][2] += w * v2;
            }
            if (writes_perm) perm[cell * perm_cols + perm_c] = bi;
        }
    }
    const size_t os = ((size_t)r * a.frames + t) * n + (size_t)c * O;
    const bool covered = s_lo <= s_hi;
#pragma unroll
    for (int o = 0; o < O; ++o) {
        out_sed[os + o] = covered ? acc_p[o] / wsum : 0.f;
        out_doa[3 * (os + o)] = covered ? acc_q[o][0] / wsum : 0.f;
        out_doa[3 * (os + o) + 1] = covered ? acc_q[o][1] / wsum : 0.f;
        out_doa[3 * (os + o) + 2] = covered ? acc_q[o][2] / wsum : 0.f;
    }
}
#undef ENS_TRY2
#undef ENS_TRY3

}  // namespace seld

using namespace seld;

extern "C" int seld_window_batch(const float* x, int64_t R, int32_t C, int32_t F, int32_t L, int32_t T, int32_t hop, int32_t S,
                                 const int32_t* table, int32_t K, int64_t m0, int32_t B, int32_t count, float* out,
                                 void* stream) {
    if (!x || !out || R <= 0 || C < 1 || C > MAP_MAX_C || F < 1 || L < 1 || T < 1 || hop < 1 || S < 1) return SELD_EINVAL;
    if (B <= 0 || count <= 0 || count > B || count > 65535) return SELD_EINVAL;
    if (K < 0 || K > MAP_MAX_K || (K > 0) != (table != nullptr)) return SELD_EINVAL;
    if ((long long)C * F * T >= (1ll << 31) || (long long)C * F * L >= (1ll << 31)) return SELD_EUNSUPPORTED;   // 32-bit offsets in a row
    if (R > (1ll << 62) / S / MAP_MAX_K) return SELD_EUNSUPPORTED;
    const long long members = (long long)R * S * (K > 0 ? K : 1);
    if (m0 < 0 || m0 > members - count) return SELD_EINVAL;
    const long long row = (long long)C * F * T;
    const long long tiles = (row + TILE_FLOATS - 1) / TILE_FLOATS, cap = TILE_MAX_BLOCKS / count > 0 ? TILE_MAX_BLOCKS / count : 1;
    const int gx = (int)(tiles < cap ? tiles : cap);
    const int vec = T % 4 == 0 && hop % 4 == 0 && L % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const WinParams a{C, F, L, T, hop, S, K, (long long)m0, vec};
    hipLaunchKernelGGL(window_batch_kernel, dim3(gx, count), dim3(TILE_THREADS), 0, (hipStream_t)stream, x, out, table, a);
    return check_launch();
}

extern "C" int seld_ensemble_combine(const float* sed, const float* doa, int64_t R, int32_t S, int32_t K, int32_t T_out,
                                     int32_t hop_out, int32_t frames, int32_t classes, int32_t overlaps, const float* win,
                                     const int32_t* table, int32_t C, int32_t align, float* out_sed, float* out_doa,
                                     int32_t* perm, void* stream) {
    if (!sed || !doa || !win || !out_sed || !out_doa) return SELD_EINVAL;
    if (R <= 0 || S < 1 || T_out < 1 || hop_out < 1 || frames < 1 || classes < 1 || overlaps < 1) return SELD_EINVAL;
    if (K < 0 || K > MAP_MAX_K || (K > 0) != (table != nullptr) || (K > 0 && (C < 1 || C > MAP_MAX_C))) return SELD_EINVAL;
    if (align != 0 && align != 1) return SELD_EINVAL;
    if ((long long)classes * overlaps > ENS_MAX_N) return SELD_EUNSUPPORTED;
    if (align && overlaps > 3) return SELD_EUNSUPPORTED;
    const bool aligned = align && overlaps > 1;                 // one slot has one pairing
    const long long reach = (long long)(S - 1) * hop_out + T_out;
    const long long t_span = perm && reach > frames ? reach : frames;
    if (t_span >= (1ll << 31)) return SELD_EUNSUPPORTED;
    const int cells = aligned ? classes : classes * overlaps;
    if (R > ((1ll << 31) - 1) * COMBINE_THREADS / (t_span * cells)) return SELD_EUNSUPPORTED;        // 2^31 workgroups or more
    const long long total = (long long)R * t_span * cells;
    const CombineParams a{(long long)R, S, K, T_out, hop_out, frames, cells, aligned ? 1 : overlaps, (int)t_span, 2 * C + 6};
    const dim3 grid((unsigned)((total + COMBINE_THREADS - 1) / COMBINE_THREADS)), block(COMBINE_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (!aligned)
        hipLaunchKernelGGL((ensemble_combine_kernel<1, false>), grid, block, 0, st, sed, doa, win, table, out_sed, out_doa, perm, a);
    else if (overlaps == 2)
        hipLaunchKernelGGL((ensemble_combine_kernel<2, true>), grid, block, 0, st, sed, doa, win, table, out_sed, out_doa, perm, a);
    else
        hipLaunchKernelGGL((ensemble_combine_kernel<3, true>), grid, block, 0, st, sed, doa, win, table, out_sed, out_doa, perm, a);
    return check_launch();
}
