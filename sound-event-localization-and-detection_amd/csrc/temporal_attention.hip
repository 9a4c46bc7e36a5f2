// Temporal attention (AT) core for gfx950: single-head flash attention over ONE projected tensor
// qkv (N, 2K + V, T) = [q (K) | k (K) | v (V)], channel-major like every TCN tensor, with a key width K and a value width V
// of their own and a mask that is a FUNCTION OF INDICES (include/seld_hip.h has the definition):
//
//   score[n,t,s] = (q[n,:,t] . k[n,:,s]) / sqrt(K)
//   allowed(n,t,s) = kind(t, s) && s < len[n]       none: true | causal: s <= t | band: |t - s| <= W
//   p = softmax of score over the allowed s;  read[n,:,t] = sum_s p[n,t,s] v[n,:,s];  lse = log sum exp over the allowed s
//
// An excluded key has weight exactly 0 (its score is -inf, not the -1e9 of seld_mha_*_ex).  A row with no allowed key
// (band together with len) gives read = 0 and lse = +inf; in backward exp(score - inf) = 0, so it contributes nothing.
//
// TILE SKIPPING.  Every kernel derives from its tile's first and last row the range [lo, hi) of the opposite index the
// mask allows (AtMask::key_range / query_range) and loops over that range only; a tile the mask boundary crosses applies
// `allowed` per element, a tile wholly inside (AtMask::whole) does not.  Key tiles at or behind len own no query: their
// dk / dv are written as zeros.  A call with no mask at all (kind none, len == T) walks its tiles in an instantiation
// of the MFMA loop without the per-tile test: the wave-uniform branch alone cost up to 28 % at T = 512.
//
// FORMS, the split of mha.hip / mha_mfma.hip:
//   valu   every 1 <= K, V <= 64 and every T.  A query (forward, dq) or a key (dk/dv) is owned by 8 lanes that split the
//          64-wide LDS tile of the other index; instantiated for max(K, V) rounded up to 8 / 16 / 32 / 48 / 64.
//   mfma   K, V each in {16, 32, 48, 64}, T % 16 == 0, every tensor on a 16-byte boundary: v_mfma_f32_16x16x4_f32, a wave
//          owns a 16-wide tile and streams the other index in 16-wide tiles from global memory one tile ahead; the first
//          product is computed transposed so that its accumulator is the B operand of the second (mha_mfma.hip explains
//          the operand layout).  SELD_MHA_NO_MFMA switches the form off.
// Backward is a delta pass (delta[n,t] = sum_d dread read), a dq kernel that owns query tiles and a dk/dv kernel that owns
// key tiles: no atomics, every sum has one owner and a fixed order, so a repeat gives the same bytes.
// Element offsets are 64-bit; a sample's workgroups are consecutive block numbers of a folded grid (AtGrid).
#include <stdio.h>
#include "common.h"
#include "env.h"
#include "mha_common.h"

namespace seld {

__device__ __forceinline__ long long at_min(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long at_max(long long a, long long b) { return a > b ? a : b; }

struct AtPlain { static constexpr bool value = false; };     // tag of a tile walk without / with the per-tile mask test
struct AtMasked { static constexpr bool value = true; };

// the index mask of one sample
struct AtMask {
    int kind, band, len;        // band <= T (clamped by the entry points); len in [1, T]
    __device__ __forceinline__ bool allowed(int t, int s) const {
        if (s >= len) return false;
        if (kind == SELD_AT_CAUSAL) return s <= t;
        if (kind == SELD_AT_BAND) return (t > s ? t - s : s - t) <= band;
        return true;
    }
    // nothing is excluded anywhere
    __device__ __forceinline__ bool plain(int T) const { return kind == SELD_AT_NONE && len == T; }
    // every (t, s) of query rows t0..t1 x keys s0..s1 is allowed
    __device__ __forceinline__ bool whole(int t0, int t1, int s0, int s1) const {
        if (s1 >= len) return false;
        if (kind == SELD_AT_CAUSAL) return s1 <= t0;
        if (kind == SELD_AT_BAND) return (long long)s1 - t0 <= band && (long long)t1 - s0 <= band;
        return true;
    }
    // [lo, hi): the keys some query of rows t0..t1 may attend
    __device__ __forceinline__ void key_range(int t0, int t1, int& lo, int& hi) const {
        long long l = 0, h = len;
        if (kind == SELD_AT_CAUSAL) h = at_min(h, (long long)t1 + 1);
        if (kind == SELD_AT_BAND) {
            l = at_max(l, (long long)t0 - band);
            h = at_min(h, (long long)t1 + band + 1);
        }
        lo = (int)l;
        hi = (int)at_max(l, h);
    }
    // [lo, hi): the queries that may attend some key of s0..s1
    __device__ __forceinline__ void query_range(int s0, int s1, int T, int& lo, int& hi) const {
        long long l = 0, h = T;
        if (s0 >= len) h = 0;
        if (kind == SELD_AT_CAUSAL) l = s0;
        if (kind == SELD_AT_BAND) {
            l = at_max(l, (long long)s0 - band);
            h = at_min(h, (long long)s1 + band + 1);
        }
        lo = (int)l;
        hi = (int)at_max(l, h);
    }
};

struct AtMaskArgs {
    int kind, band;
    const int32_t* lengths;     // nullable
    __device__ __forceinline__ AtMask of(int n, int T) const {
        int len = T;
        if (lengths) len = min(max(lengths[n], 1), T);
        return AtMask{kind, band, len};
    }
};

// A sample's `wgs` workgroups are consecutive block numbers; the `blocks` = N * wgs of them are folded into a two-dimensional
// grid, since one grid dimension holds fewer than 2^32 THREADS (16.7 M workgroups of 256): a launch beyond that is cut
// short without an error.
struct AtGrid {
    int wgs;
    unsigned blocks;
    // false: a block of the last grid row behind the end (uniform over the workgroup, tested before any barrier)
    __device__ __forceinline__ bool locate(int& n, int& blk) const {
        const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
        n = (int)(id / (unsigned)wgs);
        blk = (int)(id - (unsigned)n * (unsigned)wgs);
        return id < blocks;
    }
};
constexpr unsigned AT_GRID_X = 1u << 20;

// ======================================================================================================================
// VALU form
// ======================================================================================================================
constexpr int AT_TILE = 64;     // keys (queries) per LDS tile
constexpr int AT_OWN = 32;      // queries (keys) owned by a workgroup: 4 waves x 8

__device__ __forceinline__ float at_group8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    v = fmaxf(v, __shfl_xor(v, 4, 64));
    return v;
}
__device__ __forceinline__ float at_group8_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

template <int HDM>
__global__ __launch_bounds__(256) void at_fwd_valu_kernel(const float* __restrict__ qkv, int T, int K, int V, AtGrid grid,
                                                          AtMaskArgs ma, float* __restrict__ read, float* __restrict__ lse) {
    __shared__ float Ks[HDM][AT_TILE];
    __shared__ float Vs[HDM][AT_TILE];
    __shared__ float Os[HDM][AT_OWN + 1];
    __shared__ float Ss[AT_OWN][AT_TILE + 1];
    const int tid = threadIdx.x;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const float* qb = qkv + (size_t)n * (2 * K + V) * T;
    const float* kb = qb + (size_t)K * T;
    const float* vb = kb + (size_t)K * T;
    const int own = tid >> 3, kl = tid & 7;
    const int t0 = blk * AT_OWN;
    const int tq = t0 + own;
    const bool qok = tq < T;
    const float scale = 1.0f / sqrtf((float)K);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.key_range(t0, min(t0 + AT_OWN, T) - 1, lo, hi);
    lo -= lo % AT_TILE;

    float qv[HDM], o[HDM];
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        qv[d] = (qok && d < K) ? qb[(size_t)d * T + tq] * scale : 0.f;
        o[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;

    for (int k0 = lo; k0 < hi; k0 += AT_TILE) {
        __syncthreads();
        for (int e = tid; e < HDM * AT_TILE; e += 256) {
            const int d = e / AT_TILE, t = e - d * AT_TILE;
            const bool in = k0 + t < T;
            Ks[d][t] = (in && d < K) ? kb[(size_t)d * T + k0 + t] : 0.f;
            Vs[d][t] = (in && d < V) ? vb[(size_t)d * T + k0 + t] : 0.f;
        }
        __syncthreads();
        float tmax = -INFINITY;
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {
            const int key = kl + 8 * j;
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < HDM; ++d) acc += qv[d] * Ks[d][key];
            acc = mk.allowed(tq, k0 + key) ? acc : -INFINITY;       // len <= T: a key past T is never allowed
            Ss[own][key] = acc;                 // only this lane reads it back
            tmax = fmaxf(tmax, acc);
        }
        tmax = at_group8_max(tmax);
        const float mnew = fmaxf(m, tmax);
        const float alpha = (m == -INFINITY) ? 0.f : expf(m - mnew);
        l *= alpha;
#pragma unroll
        for (int d = 0; d < HDM; ++d) o[d] *= alpha;
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {
            const int key = kl + 8 * j;
            const float sj = Ss[own][key];
            const float p = (sj == -INFINITY) ? 0.f : expf(sj - mnew);
            l += p;
#pragma unroll
            for (int d = 0; d < HDM; ++d) o[d] += p * Vs[d][key];
        }
        m = mnew;
    }
    l = at_group8_sum(l);
    const float inv = l > 0.f ? 1.0f / l : 0.f;         // no allowed key: read = 0, lse = +inf
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        const float od = at_group8_sum(o[d]) * inv;
        if (kl == (d & 7)) Os[d][own] = od;
    }
    if (kl == 0 && qok) lse[(size_t)n * T + tq] = l > 0.f ? m + logf(l) : INFINITY;
    __syncthreads();
    float* rb = read + (size_t)n * V * T;
    for (int e = tid; e < HDM * AT_OWN; e += 256) {
        const int d = e / AT_OWN, t = e - d * AT_OWN;
        if (d < V && t0 + t < T) rb[(size_t)d * T + t0 + t] = Os[d][t];
    }
}

// delta[n][t] = sum_d dread[n][d][t] * read[n][d][t]
__global__ __launch_bounds__(256) void at_delta_kernel(const float* __restrict__ read, const float* __restrict__ dread, int T,
                                                       int V, AtGrid grid, float* __restrict__ delta) {
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const int t = blk * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t base = (size_t)n * V * T;
    float s = 0.f;
    for (int d = 0; d < V; ++d) s += read[base + (size_t)d * T + t] * dread[base + (size_t)d * T + t];
    delta[(size_t)n * T + t] = s;
}

// dq: each query owned by 8 lanes, loop over the allowed key tiles
template <int HDM>
__global__ __launch_bounds__(256) void at_bwd_dq_valu_kernel(const float* __restrict__ qkv, const float* __restrict__ dread,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             int T, int K, int V, AtGrid grid, AtMaskArgs ma,
                                                             float* __restrict__ dqkv) {
    __shared__ float Ks[HDM][AT_TILE];
    __shared__ float Vs[HDM][AT_TILE];
    __shared__ float Os[HDM][AT_OWN + 1];
    const int tid = threadIdx.x;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const float* qb = qkv + (size_t)n * (2 * K + V) * T;
    const float* kb = qb + (size_t)K * T;
    const float* vb = kb + (size_t)K * T;
    const float* gb = dread + (size_t)n * V * T;
    const int own = tid >> 3, kl = tid & 7;
    const int t0 = blk * AT_OWN;
    const int tq = t0 + own;
    const bool qok = tq < T;
    const float scale = 1.0f / sqrtf((float)K);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.key_range(t0, min(t0 + AT_OWN, T) - 1, lo, hi);
    lo -= lo % AT_TILE;
    float qv[HDM], dov[HDM], acc[HDM];
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        qv[d] = (qok && d < K) ? qb[(size_t)d * T + tq] * scale : 0.f;
        dov[d] = (qok && d < V) ? gb[(size_t)d * T + tq] : 0.f;
        acc[d] = 0.f;
    }
    const float my_lse = qok ? lse[(size_t)n * T + tq] : 0.f;
    const float my_delta = qok ? delta[(size_t)n * T + tq] : 0.f;
    for (int k0 = lo; k0 < hi; k0 += AT_TILE) {
        __syncthreads();
        for (int e = tid; e < HDM * AT_TILE; e += 256) {
            const int d = e / AT_TILE, t = e - d * AT_TILE;
            const bool in = k0 + t < T;
            Ks[d][t] = (in && d < K) ? kb[(size_t)d * T + k0 + t] : 0.f;
            Vs[d][t] = (in && d < V) ? vb[(size_t)d * T + k0 + t] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {
            const int key = kl + 8 * j;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HDM; ++d) {
                s += qv[d] * Ks[d][key];
                dp += dov[d] * Vs[d][key];
            }
            const bool live = qok && mk.allowed(tq, k0 + key);
            const float p = live ? expf(s - my_lse) : 0.f;       // lse = +inf (no allowed key): exp(-inf) = 0
            const float ds = p * (dp - my_delta) * scale;
#pragma unroll
            for (int d = 0; d < HDM; ++d) acc[d] += ds * Ks[d][key];
        }
    }
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        const float r = at_group8_sum(acc[d]);
        if (kl == (d & 7)) Os[d][own] = r;
    }
    __syncthreads();
    float* ob = dqkv + (size_t)n * (2 * K + V) * T;
    for (int e = tid; e < HDM * AT_OWN; e += 256) {
        const int d = e / AT_OWN, t = e - d * AT_OWN;
        if (d < K && t0 + t < T) ob[(size_t)d * T + t0 + t] = Os[d][t];
    }
}

// dk, dv: each key owned by 8 lanes, loop over the query tiles that may attend it
template <int HDM>
__global__ __launch_bounds__(256) void at_bwd_dkv_valu_kernel(const float* __restrict__ qkv, const float* __restrict__ dread,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              int T, int K, int V, AtGrid grid, AtMaskArgs ma,
                                                              float* __restrict__ dqkv) {
    __shared__ float Qs[HDM][AT_TILE];
    __shared__ float Ds[HDM][AT_TILE];
    __shared__ float Ls[AT_TILE], Dl[AT_TILE];
    __shared__ float Os[HDM][AT_OWN + 1];
    const int tid = threadIdx.x;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const float* qb = qkv + (size_t)n * (2 * K + V) * T;
    const float* kb = qb + (size_t)K * T;
    const float* vb = kb + (size_t)K * T;
    const float* gb = dread + (size_t)n * V * T;
    const int own = tid >> 3, ql = tid & 7;
    const int s0 = blk * AT_OWN;
    const int tk = s0 + own;
    const bool kok = tk < T;
    const float scale = 1.0f / sqrtf((float)K);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.query_range(s0, min(s0 + AT_OWN, T) - 1, T, lo, hi);
    lo -= lo % AT_TILE;
    float kv[HDM], vv[HDM], adk[HDM], adv[HDM];
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        kv[d] = (kok && d < K) ? kb[(size_t)d * T + tk] : 0.f;
        vv[d] = (kok && d < V) ? vb[(size_t)d * T + tk] : 0.f;
        adk[d] = 0.f;
        adv[d] = 0.f;
    }
    for (int q0 = lo; q0 < hi; q0 += AT_TILE) {
        __syncthreads();
        for (int e = tid; e < HDM * AT_TILE; e += 256) {
            const int d = e / AT_TILE, t = e - d * AT_TILE;
            const bool in = q0 + t < T;
            Qs[d][t] = (in && d < K) ? qb[(size_t)d * T + q0 + t] * scale : 0.f;
            Ds[d][t] = (in && d < V) ? gb[(size_t)d * T + q0 + t] : 0.f;
        }
        if (tid < AT_TILE) {
            const bool in = q0 + tid < T;
            Ls[tid] = in ? lse[(size_t)n * T + q0 + tid] : 0.f;
            Dl[tid] = in ? delta[(size_t)n * T + q0 + tid] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {
            const int qq = ql + 8 * j;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HDM; ++d) {
                s += Qs[d][qq] * kv[d];
                dp += Ds[d][qq] * vv[d];
            }
            const bool live = kok && q0 + qq < T && mk.allowed(q0 + qq, tk);
            const float p = live ? expf(s - Ls[qq]) : 0.f;
            const float ds = p * (dp - Dl[qq]);         // Qs already carries `scale`
#pragma unroll
            for (int d = 0; d < HDM; ++d) {
                adv[d] += p * Ds[d][qq];
                adk[d] += ds * Qs[d][qq];
            }
        }
    }
    float* okb = dqkv + (size_t)n * (2 * K + V) * T + (size_t)K * T;
    float* ovb = okb + (size_t)K * T;
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        const float r = at_group8_sum(adk[d]);
        if (ql == (d & 7)) Os[d][own] = r;
    }
    __syncthreads();
    for (int e = tid; e < HDM * AT_OWN; e += 256) {
        const int d = e / AT_OWN, t = e - d * AT_OWN;
        if (d < K && s0 + t < T) okb[(size_t)d * T + s0 + t] = Os[d][t];
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < HDM; ++d) {
        const float r = at_group8_sum(adv[d]);
        if (ql == (d & 7)) Os[d][own] = r;
    }
    __syncthreads();
    for (int e = tid; e < HDM * AT_OWN; e += 256) {
        const int d = e / AT_OWN, t = e - d * AT_OWN;
        if (d < V && s0 + t < T) ovb[(size_t)d * T + s0 + t] = Os[d][t];
    }
}

// ======================================================================================================================
// fp32-MFMA form (operand layout: mha_mfma.hip).  T % 16 == 0, so every 16-wide tile lies inside the tensors.
// ======================================================================================================================
template <int KD, int VD>
__global__ __launch_bounds__(256) void at_fwd_mfma_kernel(const float* __restrict__ qkv, int T, AtGrid grid, AtMaskArgs ma,
                                                          float* __restrict__ read, float* __restrict__ lse) {
    constexpr int KS = KD / 4;       // k-steps of the score's reduction
    constexpr int VT = VD / 16;      // 16-row tiles of read^T
    const int lane = threadIdx.x & 63, c = lane & 15, fk = lane >> 4;
    const int wave = threadIdx.x >> 6;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const int q0 = (blk * 4 + wave) * 16;
    if (q0 >= T) return;
    const float* qb = qkv + (size_t)n * (2 * KD + VD) * T;
    const float* kb = qb + (size_t)KD * T;
    const float* vb = kb + (size_t)KD * T;
    const float scale = 1.0f / sqrtf((float)KD);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.key_range(q0, q0 + 15, lo, hi);
    lo &= ~15;

    float qf[KS];                                            // B operand of S^T: Q[d = 4s + fk][query c], pre-scaled
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = qb[(size_t)(4 * s + fk) * T + q0 + c] * scale;
    floatx4 o[VT];
#pragma unroll
    for (int dt = 0; dt < VT; ++dt) o[dt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                            // l: this lane's share of the row sum (its 4 keys per tile)

    float ka[2][KS];                                         // A of S^T: K[d = 4s + fk][key k0 + c]
    float4 va[2][VT];                                        // A of read^T: V[d = 16dt + c][key k0 + 4fk .. +3]
    auto load_tile = [&](int k0, float (&kr)[KS], float4 (&vr)[VT]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) kr[s] = kb[(size_t)(4 * s + fk) * T + k0 + c];
#pragma unroll
        for (int dt = 0; dt < VT; ++dt) vr[dt] = *reinterpret_cast<const float4*>(vb + (size_t)(dt * 16 + c) * T + k0 + 4 * fk);
    };
    auto tile = [&](auto masked, int k0, const float (&kr)[KS], const float4 (&vr)[VT]) __attribute__((always_inline)) {
        floatx4 st = {0.f, 0.f, 0.f, 0.f};                   // S^T[key k0 + 4fk + r][query c]
#pragma unroll
        for (int s = 0; s < KS; ++s) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[s], qf[s], st, 0, 0, 0);
        if (decltype(masked)::value && !mk.whole(q0, q0 + 15, k0, k0 + 15)) {      // the mask boundary crosses this tile (wave-uniform)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[r] = mk.allowed(q0 + c, k0 + 4 * fk + r) ? st[r] : -INFINITY;
        }
        float mx = fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3]));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float mref = mn == -INFINITY ? 0.f : mn;       // no allowed key so far: every exp below is exp(-inf) = 0
        const float alpha = __expf(m - mref);
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = __expf(st[r] - mref);
        l = l * alpha + (p[0] + p[1]) + (p[2] + p[3]);
        m = mn;
#pragma unroll
        for (int dt = 0; dt < VT; ++dt) {
            o[dt] *= alpha;
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[dt].x, p[0], o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[dt].y, p[1], o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[dt].z, p[2], o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[dt].w, p[3], o[dt], 0, 0, 0);
        }
    };
    auto walk = [&](auto masked) __attribute__((always_inline)) {
        if (lo >= hi) return;
        load_tile(lo, ka[0], va[0]);
        for (int k0 = lo; k0 < hi; k0 += 32) {
            if (k0 + 16 < hi) load_tile(k0 + 16, ka[1], va[1]);
            tile(masked, k0, ka[0], va[0]);
            if (k0 + 16 >= hi) break;
            if (k0 + 32 < hi) load_tile(k0 + 32, ka[0], va[0]);
            tile(masked, k0 + 16, ka[1], va[1]);
        }
    };
    if (mk.plain(T)) walk(AtPlain{});                        // no mask at all: the loop without the per-tile test
    else walk(AtMasked{});
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = l > 0.f ? 1.0f / l : 0.f;              // no allowed key: read = 0, lse = +inf
    float* rb = read + (size_t)n * VD * T;
#pragma unroll
    for (int dt = 0; dt < VT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) rb[(size_t)(dt * 16 + 4 * fk + r) * T + q0 + c] = o[dt][r] * inv;
    if (fk == 0) lse[(size_t)n * T + q0 + c] = l > 0.f ? m + logf(l) : INFINITY;
}

template <int KD, int VD>
__global__ __launch_bounds__(256) void at_bwd_dq_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dread,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             int T, AtGrid grid, AtMaskArgs ma, float* __restrict__ dqkv) {
    constexpr int KS = KD / 4, VS = VD / 4, KT = KD / 16;
    const int lane = threadIdx.x & 63, c = lane & 15, fk = lane >> 4;
    const int wave = threadIdx.x >> 6;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const int q0 = (blk * 4 + wave) * 16;
    if (q0 >= T) return;
    const float* qb = qkv + (size_t)n * (2 * KD + VD) * T;
    const float* kb = qb + (size_t)KD * T;
    const float* vb = kb + (size_t)KD * T;
    const float* gb = dread + (size_t)n * VD * T;
    const float scale = 1.0f / sqrtf((float)KD);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.key_range(q0, q0 + 15, lo, hi);
    lo &= ~15;

    float qf[KS], gf[VS];                                    // B operands: Q (scaled), dread at [d = 4s + fk][query c]
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = qb[(size_t)(4 * s + fk) * T + q0 + c] * scale;
#pragma unroll
    for (int s = 0; s < VS; ++s) gf[s] = gb[(size_t)(4 * s + fk) * T + q0 + c];
    const float my_lse = lse[(size_t)n * T + q0 + c];
    const float my_delta = delta[(size_t)n * T + q0 + c];
    floatx4 acc[KT];
#pragma unroll
    for (int dt = 0; dt < KT; ++dt) acc[dt] = (floatx4){0.f, 0.f, 0.f, 0.f};

    float ka[2][KS], va[2][VS];                              // A of S^T / dP^T: K, V at [d = 4s + fk][key k0 + c]
    float4 kk[2][KT];                                        // A of dq^T: K[d = 16dt + c][key k0 + 4fk .. +3]
    auto load_tile = [&](int k0, float (&kr)[KS], float (&vr)[VS], float4 (&k4)[KT]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) kr[s] = kb[(size_t)(4 * s + fk) * T + k0 + c];
#pragma unroll
        for (int s = 0; s < VS; ++s) vr[s] = vb[(size_t)(4 * s + fk) * T + k0 + c];
#pragma unroll
        for (int dt = 0; dt < KT; ++dt) k4[dt] = *reinterpret_cast<const float4*>(kb + (size_t)(dt * 16 + c) * T + k0 + 4 * fk);
    };
    auto tile = [&](auto masked, int k0, const float (&kr)[KS], const float (&vr)[VS], const float4 (&k4)[KT])
                    __attribute__((always_inline)) {
        floatx4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};     // S^T, dP^T [key k0 + 4fk + r][query c]
#pragma unroll
        for (int s = 0; s < KS; ++s) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[s], qf[s], st, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < VS; ++s) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[s], gf[s], dp, 0, 0, 0);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = __expf(st[r] - my_lse) * (dp[r] - my_delta) * scale;
        if (decltype(masked)::value && !mk.whole(q0, q0 + 15, k0, k0 + 15)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[r] = mk.allowed(q0 + c, k0 + 4 * fk + r) ? ds[r] : 0.f;
        }
#pragma unroll
        for (int dt = 0; dt < KT; ++dt) {
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[dt].x, ds[0], acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[dt].y, ds[1], acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[dt].z, ds[2], acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[dt].w, ds[3], acc[dt], 0, 0, 0);
        }
    };
    auto walk = [&](auto masked) __attribute__((always_inline)) {
        if (lo >= hi) return;
        load_tile(lo, ka[0], va[0], kk[0]);
        for (int k0 = lo; k0 < hi; k0 += 32) {
            if (k0 + 16 < hi) load_tile(k0 + 16, ka[1], va[1], kk[1]);
            tile(masked, k0, ka[0], va[0], kk[0]);
            if (k0 + 16 >= hi) break;
            if (k0 + 32 < hi) load_tile(k0 + 32, ka[0], va[0], kk[0]);
            tile(masked, k0 + 16, ka[1], va[1], kk[1]);
        }
    };
    if (mk.plain(T)) walk(AtPlain{});
    else walk(AtMasked{});
    float* ob = dqkv + (size_t)n * (2 * KD + VD) * T;
#pragma unroll
    for (int dt = 0; dt < KT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) ob[(size_t)(dt * 16 + 4 * fk + r) * T + q0 + c] = acc[dt][r];
}

template <int KD, int VD>
__global__ __launch_bounds__(256) void at_bwd_dkv_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dread,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              int T, AtGrid grid, AtMaskArgs ma, float* __restrict__ dqkv) {
    constexpr int KS = KD / 4, VS = VD / 4, KT = KD / 16, VT = VD / 16;
    const int lane = threadIdx.x & 63, c = lane & 15, fk = lane >> 4;
    const int wave = threadIdx.x >> 6;
    int n, blk;
    if (!grid.locate(n, blk)) return;
    const int k0 = (blk * 4 + wave) * 16;
    if (k0 >= T) return;
    const float* qb = qkv + (size_t)n * (2 * KD + VD) * T;
    const float* kb = qb + (size_t)KD * T;
    const float* vb = kb + (size_t)KD * T;
    const float* gb = dread + (size_t)n * VD * T;
    const float* lb = lse + (size_t)n * T;
    const float* db = delta + (size_t)n * T;
    const float scale = 1.0f / sqrtf((float)KD);
    const AtMask mk = ma.of(n, T);
    int lo, hi;
    mk.query_range(k0, k0 + 15, T, lo, hi);
    lo &= ~15;

    float kf[KS], vf[VS];                                    // B operands: K, V at [d = 4s + fk][key c]
#pragma unroll
    for (int s = 0; s < KS; ++s) kf[s] = kb[(size_t)(4 * s + fk) * T + k0 + c];
#pragma unroll
    for (int s = 0; s < VS; ++s) vf[s] = vb[(size_t)(4 * s + fk) * T + k0 + c];
    floatx4 ak[KT], av[VT];                                  // dk^T, dv^T [d = 16dt + 4fk + r][key c]
#pragma unroll
    for (int dt = 0; dt < KT; ++dt) ak[dt] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < VT; ++dt) av[dt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    // operands of the first two products (S, dP) of a query tile one tile ahead; those of the last two (dv, dk) at the top
    // of their own tile (mha_mfma.hip: two stages of everything do not fit the register file)
    struct QTile {
        float aq[KS], ag[VS];                                // A of S / dP: Q, dread at [d = 4s + fk][query q0 + c]
        float4 ls, dl;                                       // lse, delta of queries q0 + 4fk .. +3
    };
    QTile qt[2];
    auto load_tile = [&](int q0, QTile& t) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) t.aq[s] = qb[(size_t)(4 * s + fk) * T + q0 + c];
#pragma unroll
        for (int s = 0; s < VS; ++s) t.ag[s] = gb[(size_t)(4 * s + fk) * T + q0 + c];
        t.ls = *reinterpret_cast<const float4*>(lb + q0 + 4 * fk);
        t.dl = *reinterpret_cast<const float4*>(db + q0 + 4 * fk);
    };
    auto tile = [&](auto masked, int q0, const QTile& t) __attribute__((always_inline)) {
        float4 gg[VT], qq[KT];                               // A of dv^T / dk^T: dread, Q at [d = 16dt + c][query q0 + 4fk .. +3]
#pragma unroll
        for (int dt = 0; dt < VT; ++dt) gg[dt] = *reinterpret_cast<const float4*>(gb + (size_t)(dt * 16 + c) * T + q0 + 4 * fk);
#pragma unroll
        for (int dt = 0; dt < KT; ++dt) qq[dt] = *reinterpret_cast<const float4*>(qb + (size_t)(dt * 16 + c) * T + q0 + 4 * fk);
        __builtin_amdgcn_sched_barrier(0);       // (left alone the compiler sinks each of these loads to just before its MFMAs)
        floatx4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};     // S, dP [query q0 + 4fk + r][key c]
#pragma unroll
        for (int s = 0; s < KS; ++s) st = __builtin_amdgcn_mfma_f32_16x16x4f32(t.aq[s] * scale, kf[s], st, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < VS; ++s) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(t.ag[s], vf[s], dp, 0, 0, 0);
        float p[4], ds[4];
        p[0] = __expf(st[0] - t.ls.x); p[1] = __expf(st[1] - t.ls.y); p[2] = __expf(st[2] - t.ls.z); p[3] = __expf(st[3] - t.ls.w);
        if (decltype(masked)::value && !mk.whole(q0, q0 + 15, k0, k0 + 15)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = mk.allowed(q0 + 4 * fk + r, k0 + c) ? p[r] : 0.f;
        }
        ds[0] = p[0] * (dp[0] - t.dl.x) * scale; ds[1] = p[1] * (dp[1] - t.dl.y) * scale;
        ds[2] = p[2] * (dp[2] - t.dl.z) * scale; ds[3] = p[3] * (dp[3] - t.dl.w) * scale;
#pragma unroll
        for (int dt = 0; dt < VT; ++dt) {
            av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gg[dt].x, p[0], av[dt], 0, 0, 0);
            av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gg[dt].y, p[1], av[dt], 0, 0, 0);
            av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gg[dt].z, p[2], av[dt], 0, 0, 0);
            av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gg[dt].w, p[3], av[dt], 0, 0, 0);
        }
#pragma unroll
        for (int dt = 0; dt < KT; ++dt) {
            ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[dt].x, ds[0], ak[dt], 0, 0, 0);
            ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[dt].y, ds[1], ak[dt], 0, 0, 0);
            ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[dt].z, ds[2], ak[dt], 0, 0, 0);
            ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[dt].w, ds[3], ak[dt], 0, 0, 0);
        }
    };
    auto walk = [&](auto masked) __attribute__((always_inline)) {
        if (lo >= hi) return;
        load_tile(lo, qt[0]);
        for (int q0 = lo; q0 < hi; q0 += 32) {
            if (q0 + 16 < hi) load_tile(q0 + 16, qt[1]);
            tile(masked, q0, qt[0]);
            if (q0 + 16 >= hi) break;
            if (q0 + 32 < hi) load_tile(q0 + 32, qt[0]);
            tile(masked, q0 + 16, qt[1]);
        }
    };
    if (mk.plain(T)) walk(AtPlain{});
    else walk(AtMasked{});
    float* okb = dqkv + (size_t)n * (2 * KD + VD) * T + (size_t)KD * T;
    float* ovb = okb + (size_t)KD * T;
#pragma unroll
    for (int dt = 0; dt < KT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) okb[(size_t)(dt * 16 + 4 * fk + r) * T + k0 + c] = ak[dt][r];
#pragma unroll
    for (int dt = 0; dt < VT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) ovb[(size_t)(dt * 16 + 4 * fk + r) * T + k0 + c] = av[dt][r];
}

// ======================================================================================================================
// selection and launch
// ======================================================================================================================
struct AtCall {
    const float *qkv, *read, *dread, *lse, *delta;
    float *read_out, *lse_out, *dqkv;
    int N, T, K, V;
    AtMaskArgs ma;
    hipStream_t st;
};

static bool at_width_ok(int w) { return w == 16 || w == 32 || w == 48 || w == 64; }
static bool at_mfma_shape(int T, int K, int V) { return at_width_ok(K) && at_width_ok(V) && T % 16 == 0 && !env().mha_no_mfma; }
static bool at_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int at_valu_hdm(int K, int V) {
    const int w = K > V ? K : V;
    return w <= 8 ? 8 : w <= 16 ? 16 : w <= 32 ? 32 : w <= 48 ? 48 : 64;
}
// workgroups of 256 threads per sample, each owning `own` positions; blocks == 0: more than 2^31 - 1 of them
static AtGrid at_grid(int N, int T, int own) {
    const long long wgs = ((long long)T + own - 1) / own;
    return AtGrid{(int)wgs, wgs * N > 0x7fffffffLL ? 0u : (unsigned)(wgs * N)};
}
static dim3 at_dim(const AtGrid& g) {
    const unsigned x = g.blocks < AT_GRID_X ? g.blocks : AT_GRID_X;
    return dim3(x, (g.blocks + x - 1) / x);
}

enum { AT_OP_FWD = SELD_AT_FWD, AT_OP_DQ = SELD_AT_BWD_DQ, AT_OP_DKV = SELD_AT_BWD_DKV };

template <int KD, int VD>
static int at_mfma_launch(int op, const AtCall& a) {
    const AtGrid g = at_grid(a.N, a.T, 64);
    const dim3 grid = at_dim(g), block(256);
    if (op == AT_OP_FWD)
        hipLaunchKernelGGL((at_fwd_mfma_kernel<KD, VD>), grid, block, 0, a.st, a.qkv, a.T, g, a.ma, a.read_out, a.lse_out);
    else if (op == AT_OP_DQ)
        hipLaunchKernelGGL((at_bwd_dq_mfma_kernel<KD, VD>), grid, block, 0, a.st, a.qkv, a.dread, a.lse, a.delta, a.T, g,
                           a.ma, a.dqkv);
    else
        hipLaunchKernelGGL((at_bwd_dkv_mfma_kernel<KD, VD>), grid, block, 0, a.st, a.qkv, a.dread, a.lse, a.delta, a.T, g,
                           a.ma, a.dqkv);
    return check_launch();
}
template <int KD>
static int at_mfma_v(int op, const AtCall& a) {
    if (a.V == 16) return at_mfma_launch<KD, 16>(op, a);
    if (a.V == 32) return at_mfma_launch<KD, 32>(op, a);
    if (a.V == 48) return at_mfma_launch<KD, 48>(op, a);
    return at_mfma_launch<KD, 64>(op, a);
}
static int at_mfma(int op, const AtCall& a) {
    if (a.K == 16) return at_mfma_v<16>(op, a);
    if (a.K == 32) return at_mfma_v<32>(op, a);
    if (a.K == 48) return at_mfma_v<48>(op, a);
    return at_mfma_v<64>(op, a);
}

template <int HDM>
static int at_valu_launch(int op, const AtCall& a) {
    const AtGrid g = at_grid(a.N, a.T, AT_OWN);
    const dim3 grid = at_dim(g), block(256);
    if (op == AT_OP_FWD)
        hipLaunchKernelGGL((at_fwd_valu_kernel<HDM>), grid, block, 0, a.st, a.qkv, a.T, a.K, a.V, g, a.ma, a.read_out,
                           a.lse_out);
    else if (op == AT_OP_DQ)
        hipLaunchKernelGGL((at_bwd_dq_valu_kernel<HDM>), grid, block, 0, a.st, a.qkv, a.dread, a.lse, a.delta, a.T, a.K, a.V,
                           g, a.ma, a.dqkv);
    else
        hipLaunchKernelGGL((at_bwd_dkv_valu_kernel<HDM>), grid, block, 0, a.st, a.qkv, a.dread, a.lse, a.delta, a.T, a.K, a.V,
                           g, a.ma, a.dqkv);
    return check_launch();
}
static int at_valu(int op, const AtCall& a) {
    switch (at_valu_hdm(a.K, a.V)) {
        case 8: return at_valu_launch<8>(op, a);
        case 16: return at_valu_launch<16>(op, a);
        case 32: return at_valu_launch<32>(op, a);
        case 48: return at_valu_launch<48>(op, a);
        default: return at_valu_launch<64>(op, a);
    }
}

// SELD_OK, or the refusal of a call's sizes and mask (before anything is written)
static int at_args(int32_t N, int32_t T, int32_t K, int32_t V, int32_t mask_kind, int32_t band) {
    if (N <= 0 || T <= 0 || K <= 0 || V <= 0 || band < 0) return SELD_EINVAL;
    if (mask_kind != SELD_AT_NONE && mask_kind != SELD_AT_CAUSAL && mask_kind != SELD_AT_BAND) return SELD_EINVAL;
    if (K > SELD_AT_MAX_WIDTH || V > SELD_AT_MAX_WIDTH) return SELD_EUNSUPPORTED;
    if (!at_grid(N, T, AT_OWN).blocks) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

}  // namespace seld
using namespace seld;

extern "C" int seld_at_fwd(const float* qkv, int32_t N, int32_t T, int32_t K, int32_t V, int32_t mask_kind, int32_t band,
                           const int32_t* lengths, float* read, float* lse, void* stream) {
    if (!qkv || !read || !lse) return SELD_EINVAL;
    int rc = at_args(N, T, K, V, mask_kind, band);
    if (rc) return rc;
    AtCall a{};
    a.qkv = qkv; a.read_out = read; a.lse_out = lse;
    a.N = N; a.T = T; a.K = K; a.V = V;
    a.ma = AtMaskArgs{mask_kind, band < T ? band : T, lengths};
    a.st = (hipStream_t)stream;
    if (at_mfma_shape(T, K, V) && at_aligned(qkv) && at_aligned(read) && at_aligned(lse)) return at_mfma(AT_OP_FWD, a);
    return at_valu(AT_OP_FWD, a);
}

extern "C" size_t seld_at_bwd_workspace(int32_t N, int32_t T) {
    if (N <= 0 || T <= 0) return 0;
    return (size_t)N * T * sizeof(float);
}

extern "C" int seld_at_bwd(const float* qkv, const float* read, const float* dread, const float* lse, int32_t N, int32_t T,
                           int32_t K, int32_t V, int32_t mask_kind, int32_t band, const int32_t* lengths, float* dqkv,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!qkv || !read || !dread || !lse || !dqkv) return SELD_EINVAL;
    int rc = at_args(N, T, K, V, mask_kind, band);
    if (rc) return rc;
    if (!workspace || workspace_bytes < seld_at_bwd_workspace(N, T)) return SELD_EWORKSPACE;
    AtCall a{};
    a.qkv = qkv; a.read = read; a.dread = dread; a.lse = lse; a.dqkv = dqkv;
    a.delta = (const float*)workspace;
    a.N = N; a.T = T; a.K = K; a.V = V;
    a.ma = AtMaskArgs{mask_kind, band < T ? band : T, lengths};
    a.st = (hipStream_t)stream;
    const AtGrid dg = at_grid(N, T, 256);
    hipLaunchKernelGGL(at_delta_kernel, at_dim(dg), dim3(256), 0, a.st, read, dread, T, V, dg, (float*)workspace);
    rc = check_launch();
    if (rc) return rc;
    const bool mfma = at_mfma_shape(T, K, V) && at_aligned(qkv) && at_aligned(dread) && at_aligned(lse) &&
                      at_aligned(workspace) && at_aligned(dqkv);
    rc = mfma ? at_mfma(AT_OP_DQ, a) : at_valu(AT_OP_DQ, a);
    if (rc) return rc;
    return mfma ? at_mfma(AT_OP_DKV, a) : at_valu(AT_OP_DKV, a);
}

extern "C" int seld_at_kernel_label(int32_t op, int32_t T, int32_t K, int32_t V, char* buf, int32_t buflen) {
    static const char* const names[] = {"at_fwd", "at_bwd_dq", "at_bwd_dkv"};
    if (op < 0 || op > SELD_AT_BWD_DKV || !buf || buflen < 48) return SELD_EINVAL;
    int rc = at_args(1, T, K, V, SELD_AT_NONE, 0);
    if (rc) return rc;
    if (at_mfma_shape(T, K, V)) snprintf(buf, buflen, "%s_mfma_kernel<%d,%d>", names[op], K, V);
    else snprintf(buf, buflen, "%s_valu_kernel<%d>", names[op], at_valu_hdm(K, V));
    return SELD_OK;
}
