// BatchNorm statistics, BatchNorm + fused activation and the gated activation for gfx950.  All HBM-bound: 16-byte
// loads/stores along the contiguous S axis, per-channel reductions by wave shuffles + one atomic per wave (guide:
// Appendix B "Reduction").  Each formula has one definition (bn_* / gate_* cores); the element-walk, row and channel
// kernels differ in how they walk, stage loads and reduce, not in what they compute per element.
#include <cstdio>
#include <type_traits>

#include "env.h"
#include "nn_common.h"

namespace seld {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ------------------------------------------------------------------------------------------
// per-channel sum / sum of squares over (N, S)
// grid: (chunks, C); each block walks `chunk` elements of channel c's N*S index space.
// ------------------------------------------------------------------------------------------
constexpr int RED_CHUNK = 8192;

template <typename F>
__device__ __forceinline__ void channel_walk(int N, int C, int S, int c, F&& f) {
    // calls f(offset_of_4_or_1_elements, count) for this block's slice of channel c
    const long long M = (long long)N * S;
    const long long chunk = gridDim.x == 1 ? M : RED_CHUNK;      // one workgroup per channel (SELD_DETERMINISTIC): the whole range
    const long long beg = (long long)blockIdx.x * chunk;
    long long end = beg + chunk;
    if (end > M) end = M;
    if ((S & 3) == 0) {
        for (long long i = beg + (long long)threadIdx.x * 4; i < end; i += (long long)blockDim.x * 4) {
            long long n = i / S;
            int s = (int)(i - n * S);
            f(((size_t)n * C + c) * S + s, 4);
        }
    } else {
        for (long long i = beg + threadIdx.x; i < end; i += blockDim.x) {
            long long n = i / S;
            int s = (int)(i - n * S);
            f(((size_t)n * C + c) * S + s, 1);
        }
    }
}

template <int NV>
__device__ __forceinline__ void block_atomic(float (&v)[NV], float* const (&dst)[NV]) {
    __shared__ float red[NV][4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int k = threadIdx.x;
        atomicAdd(dst[k], red[k][0] + red[k][1] + red[k][2] + red[k][3]);
    }
}

__global__ __launch_bounds__(256) void channel_stats_kernel(const float* __restrict__ x, int N, int C, int S,
                                                            float* __restrict__ stats) {
    const int c = blockIdx.y;
    float v[2] = {0.f, 0.f};
    channel_walk(N, C, S, c, [&](size_t off, int cnt) {
        if (cnt == 4) {
            float4 a = ld4(x + off);
            v[0] += (a.x + a.y) + (a.z + a.w);
            v[1] += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
        } else {
            float a = x[off];
            v[0] += a;
            v[1] += a * a;
        }
    });
    float* rep = stats + (size_t)(blockIdx.x % SELD_STATS_REPLICAS) * 2 * C;
    float* const dst[2] = {rep + c, rep + C + c};
    block_atomic<2>(v, dst);
}

// One WAVE per channel: lane r owns replica row r (SELD_STATS_REPLICAS == 64), the 64 partial sums are added in fp64
// with a shuffle tree.  (A thread per channel walking the 64 rows took 8 us -- per BatchNorm, 33 times a step.)
struct BnFin {
    float* stats; float* mean; float* invstd; float* rmean; float* rvar; long long* nbt;
};
// (`f` is a reference to the pointer on purpose: handed the pointer itself, the compiler loads the six pointers of BOTH
// layers in bn_finalize2_kernel and selects each, 32 SGPRs against 22; this way it selects the argument block's address
// once and loads what it uses)
__device__ __forceinline__ void bn_finalize_layer(const BnFin* const& f, int C, double count, float eps, float momentum, int clear) {
    static_assert(SELD_STATS_REPLICAS == 64, "one lane per replica row");
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0 && f->nbt) *f->nbt += 1;      // num_batches_tracked (torch.nn.BatchNorm bookkeeping)
    if (c >= C) return;
    float* p1 = f->stats + (size_t)lane * 2 * C + c;
    float* p2 = p1 + C;
    double s1 = (double)*p1, s2 = (double)*p2;
    if (clear) { *p1 = 0.f; *p2 = 0.f; }                              // hand the buffer back zeroed (pooled by the host mirror)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if (lane != 0) return;
    const double m = s1 / count;
    double var = s2 / count - m * m;
    if (var < 0.0) var = 0.0;
    f->mean[c] = (float)m;
    f->invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (f->rmean) f->rmean[c] = (1.f - momentum) * f->rmean[c] + momentum * (float)m;
    if (f->rvar) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        f->rvar[c] = (1.f - momentum) * f->rvar[c] + momentum * (float)unbiased;
    }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(float* __restrict__ stats, int C, double count, float eps,
                                                          float momentum, float* __restrict__ mean,
                                                          float* __restrict__ invstd, float* __restrict__ rmean,
                                                          float* __restrict__ rvar, long long* __restrict__ nbt, int clear) {
    const BnFin f{stats, mean, invstd, rmean, rvar, nbt};
    const BnFin* const p = &f;
    bn_finalize_layer(p, C, count, eps, momentum, clear);
}

// Two BatchNorms of the same channel count in one launch (the gate's batch_filter2 / batch_gate2, whose statistics come
// from one pair convolution): blockIdx.y selects the layer.
__global__ __launch_bounds__(256) void bn_finalize2_kernel(BnFin a, BnFin b, int C, double count, float eps, float momentum, int clear) {
    const BnFin* const p = blockIdx.y ? &b : &a;
    bn_finalize_layer(p, C, count, eps, momentum, clear);
}

// eval mode: mean = running_mean, invstd = rsqrt(running_var + eps)
__global__ void bn_eval_stats_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar, int C, float eps,
                                     float* __restrict__ mean, float* __restrict__ invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mean[c] = rmean[c];
    invstd[c] = 1.0f / sqrtf(rvar[c] + eps);
}

// ------------------------------------------------------------------------------------------
// elementwise over (N, C, S) with per-channel constants
// ------------------------------------------------------------------------------------------
template <typename F>
__device__ __forceinline__ void ncs_walk(long long total, int C, int S, F&& f) {
    // grid-stride over groups of 4 (S % 4 == 0) or single elements
    if ((S & 3) == 0) {
        const long long groups = total >> 2;
        for (long long gidx = (long long)blockIdx.x * blockDim.x + threadIdx.x; gidx < groups;
             gidx += (long long)gridDim.x * blockDim.x) {
            const long long i = gidx << 2;
            const int c = (int)((i / S) % C);
            f((size_t)i, c, 4);
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
             i += (long long)gridDim.x * blockDim.x) {
            const int c = (int)((i / S) % C);
            f((size_t)i, c, 1);
        }
    }
}

// ---- BatchNorm + activation, per element.  y = act(x * a + b) with a = gamma * invstd, b = beta - mean * a; backward
// from dz = dy * act'(y) and xhat = (x - mean) * invstd: dx = a * (dz - mean(dz) - xhat * mean(dz * xhat)).
__device__ __forceinline__ float bn_y(float x, float a, float b, int act) { return act_apply(x * a + b, act); }
__device__ __forceinline__ float bn_dz(float dy, float y, int act) { return dy * act_grad_from_y(y, act); }
__device__ __forceinline__ float bn_xhat(float x, float mu, float is) { return (x - mu) * is; }
__device__ __forceinline__ float bn_dx(float a, float dz, float xhat, float k1, float k2) { return a * (dz - k1 - xhat * k2); }

__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ x, long long total, int C, int S,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int act, float* __restrict__ y) {
    ncs_walk(total, C, S, [&](size_t i, int c, int cnt) {
        const float a = gamma[c] * invstd[c];
        const float b = beta[c] - mean[c] * a;
        if (cnt == 4) {
            const float4 v = ld4(x + i);
            *reinterpret_cast<float4*>(y + i) =
                make_float4(bn_y(v.x, a, b, act), bn_y(v.y, a, b, act), bn_y(v.z, a, b, act), bn_y(v.w, a, b, act));
        } else {
            y[i] = bn_y(x[i], a, b, act);
        }
    });
}

// (the sums take dz * (x - mu) * is in that order, not dz * xhat: the summands' bits are part of the kernel's contract)
__global__ __launch_bounds__(256) void bn_act_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ y, int N, int C, int S,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, int act,
                                                                float* __restrict__ red) {
    const int c = blockIdx.y;
    const float mu = mean[c], is = invstd[c];
    float v[2] = {0.f, 0.f};   // dgamma, dbeta
    channel_walk(N, C, S, c, [&](size_t off, int cnt) {
        if (cnt == 4) {
            const float4 g = ld4(dy + off), xx = ld4(x + off), yy = ld4(y + off);
            float d0 = bn_dz(g.x, yy.x, act), d1 = bn_dz(g.y, yy.y, act);
            float d2 = bn_dz(g.z, yy.z, act), d3 = bn_dz(g.w, yy.w, act);
            v[0] += d0 * (xx.x - mu) * is + d1 * (xx.y - mu) * is + d2 * (xx.z - mu) * is + d3 * (xx.w - mu) * is;
            v[1] += (d0 + d1) + (d2 + d3);
        } else {
            float d = bn_dz(dy[off], y[off], act);
            v[0] += d * (x[off] - mu) * is;
            v[1] += d;
        }
    });
    float* const dst[2] = {red + c, red + C + c};
    block_atomic<2>(v, dst);
}

__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ y, long long total, int C, int S,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, int act,
                                                               const float* __restrict__ red, float inv_count, int train,
                                                               float* __restrict__ dx) {
    ncs_walk(total, C, S, [&](size_t i, int c, int cnt) {
        const float mu = mean[c], is = invstd[c];
        const float a = gamma[c] * is;
        const float k1 = train ? red[C + c] * inv_count : 0.f;       // mean(dz)
        const float k2 = train ? red[c] * inv_count : 0.f;           // mean(dz * xhat)
        auto one = [&](float g, float xx, float yy) { return bn_dx(a, bn_dz(g, yy, act), bn_xhat(xx, mu, is), k1, k2); };
        if (cnt == 4) {
            const float4 g = ld4(dy + i), xx = ld4(x + i), yy = ld4(y + i);
            float4 o = make_float4(one(g.x, xx.x, yy.x), one(g.y, xx.y, yy.y), one(g.z, xx.z, yy.z), one(g.w, xx.w, yy.w));
            *reinterpret_cast<float4*>(dx + i) = o;
        } else {
            dx[i] = one(dy[i], x[i], y[i]);
        }
    });
}

// tanh and the logistic function of the gate on the hardware exponential and reciprocal (v_exp_f32 / v_rcp_f32, 1 ulp
// each): absolute error < 3e-7 over the whole range, a handful of instructions instead of the ~45 of libm's tanhf -- the
// one-pass channel backward was VALU-bound on it (3370 VALU instructions per wave, 40 us per launch ten times a step).
// Forward and backward use the same two functions.
__device__ __forceinline__ float gate_sig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float gate_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// ------------------------------------------------------------------------------------------
// gated activation  y = tanh(bn_f(yf)) * sigmoid(bn_g(yg)) * mask[n,c]
// ------------------------------------------------------------------------------------------
struct GateBN {
    const float *mean_f, *invstd_f, *gamma_f, *beta_f;
    const float *mean_g, *invstd_g, *gamma_g, *beta_g;
};

// one channel's constants of the two BatchNorms: z = x * a + b, xhat = (x - mu) * is
struct GateCh { float muf, isf, af, bf, mug, isg, ag, bg; };
__device__ __forceinline__ GateCh gate_ch(const GateBN& bn, int c) {
    GateCh k;
    k.muf = bn.mean_f[c]; k.isf = bn.invstd_f[c]; k.af = bn.gamma_f[c] * k.isf; k.bf = bn.beta_f[c] - k.muf * k.af;
    k.mug = bn.mean_g[c]; k.isg = bn.invstd_g[c]; k.ag = bn.gamma_g[c] * k.isg; k.bg = bn.beta_g[c] - k.mug * k.ag;
    return k;
}

// ---- the gate per element.  A GatePair holds one value of the filter (tanh) branch and one of the gate (sigmoid) branch.
struct GatePair { float f, g; };
// (tanh(bn_f(f)), sigmoid(bn_g(g)))
__device__ __forceinline__ GatePair gate_ts(const GateCh& k, float f, float g) {
    return {gate_tanh(f * k.af + k.bf), gate_sig(g * k.ag + k.bg)};
}
__device__ __forceinline__ float gate_y(const GateCh& k, float f, float g, float mk) {
    const GatePair a = gate_ts(k, f, g);
    return a.f * a.g * mk;
}
// gradients w.r.t. the two BatchNorm outputs
__device__ __forceinline__ GatePair gate_dz(const GateCh& k, float f, float g, float dy, float mk) {
    const GatePair a = gate_ts(k, f, g);
    const float t = a.f, s = a.g, d = dy * mk;
    return {d * s * (1.f - t * t), d * t * s * (1.f - s)};
}
// the batch means of a channel's dz (k1) and dz * xhat (k2), per branch; all zero in eval mode
struct GateMeans { float kf1, kf2, kg1, kg2; };
__device__ __forceinline__ GateMeans gate_means(const float* __restrict__ red, int C, int c, float inv_count, int train) {
    GateMeans m;
    m.kf2 = train ? red[c] * inv_count : 0.f; m.kf1 = train ? red[C + c] * inv_count : 0.f;
    m.kg2 = train ? red[2 * C + c] * inv_count : 0.f; m.kg1 = train ? red[3 * C + c] * inv_count : 0.f;
    return m;
}
// gradients w.r.t. the two BatchNorm inputs; xhat = (bn_xhat(f, muf, isf), bn_xhat(g, mug, isg))
__device__ __forceinline__ GatePair gate_dx(const GateCh& k, GatePair dz, GatePair xhat, const GateMeans& m) {
    return {k.af * (dz.f - m.kf1 - xhat.f * m.kf2), k.ag * (dz.g - m.kg1 - xhat.g * m.kg2)};
}
// one element's terms of (dgamma_f, dbeta_f, dgamma_g, dbeta_g) in the two-pass reduce kernels (dz * (x - mu) * is in
// that order, not dz * xhat: the summands' bits are part of the kernels' contract)
__device__ __forceinline__ void gate_red_add(float& v0, float& v1, float& v2, float& v3, const GateCh& k, GatePair dz,
                                             float f, float g) {
    v0 += dz.f * (f - k.muf) * k.isf;
    v1 += dz.f;
    v2 += dz.g * (g - k.mug) * k.isg;
    v3 += dz.g;
}

__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ yf, const float* __restrict__ yg,
                                                       long long total, int C, int S, GateBN bn,
                                                       const float* __restrict__ mask, float* __restrict__ y) {
    ncs_walk(total, C, S, [&](size_t i, int c, int cnt) {
        const GateCh k = gate_ch(bn, c);
        const float mk = mask ? mask[i / S] : 1.0f;
        if (cnt == 4) {
            const float4 f = ld4(yf + i), g = ld4(yg + i);
            *reinterpret_cast<float4*>(y + i) =
                make_float4(gate_y(k, f.x, g.x, mk), gate_y(k, f.y, g.y, mk), gate_y(k, f.z, g.z, mk), gate_y(k, f.w, g.w, mk));
        } else {
            y[i] = gate_y(k, yf[i], yg[i], mk);
        }
    });
}

__global__ __launch_bounds__(256) void gate_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ yf,
                                                              const float* __restrict__ yg, int N, int C, int S,
                                                              GateBN bn, const float* __restrict__ mask,
                                                              float* __restrict__ red) {
    const int c = blockIdx.y;
    const GateCh k = gate_ch(bn, c);
    float v[4] = {0.f, 0.f, 0.f, 0.f};   // dgamma_f, dbeta_f, dgamma_g, dbeta_g
    channel_walk(N, C, S, c, [&](size_t i, int cnt) {
        for (int e = 0; e < cnt; ++e) {
            const size_t off = i + e;
            const float mk = mask ? mask[off / S] : 1.0f;
            const float f = yf[off], g = yg[off];
            gate_red_add(v[0], v[1], v[2], v[3], k, gate_dz(k, f, g, dy[off], mk), f, g);
        }
    });
    float* const dst[4] = {red + c, red + C + c, red + 2 * C + c, red + 3 * C + c};
    block_atomic<4>(v, dst);
}

__global__ __launch_bounds__(256) void gate_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ yf,
                                                             const float* __restrict__ yg, long long total, int C, int S,
                                                             GateBN bn, const float* __restrict__ mask,
                                                             const float* __restrict__ red, float inv_count, int train,
                                                             float* __restrict__ dyf, float* __restrict__ dyg) {
    ncs_walk(total, C, S, [&](size_t i, int c, int cnt) {
        const GateCh k = gate_ch(bn, c);
        const GateMeans m = gate_means(red, C, c, inv_count, train);
        const float mk = mask ? mask[i / S] : 1.0f;
        for (int e = 0; e < cnt; ++e) {
            const size_t off = i + e;
            const float f = yf[off], g = yg[off];
            const GatePair o = gate_dx(k, gate_dz(k, f, g, dy[off], mk), {bn_xhat(f, k.muf, k.isf), bn_xhat(g, k.mug, k.isg)}, m);
            dyf[off] = o.f;
            dyg[off] = o.g;
        }
    });
}

// ---- row forms (S % 4 == 0): one WAVE per (n, c) row -- the channel's constants are scalar loads, no index
// division per element, every access 16 bytes.  (The element-walk forms above spend a 64-bit division and eight
// constant loads per 4 elements: 33-37 us for a 12.6 MB TCN tensor, these run in about half.)

__global__ __launch_bounds__(256) void gate_fwd_row_kernel(const float* __restrict__ yf, const float* __restrict__ yg,
                                                           int rows, int C, int S, GateBN bn,
                                                           const float* __restrict__ mask, float* __restrict__ y) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const GateCh k = gate_ch(bn, row % C);
        const float mk = mask ? mask[row] : 1.0f;
        const size_t base = (size_t)row * S;
        for (int s = lane * 4; s < S; s += 256) {
            const float4 f = ld4(yf + base + s), g = ld4(yg + base + s);
            *reinterpret_cast<float4*>(y + base + s) =
                make_float4(gate_y(k, f.x, g.x, mk), gate_y(k, f.y, g.y, mk), gate_y(k, f.z, g.z, mk), gate_y(k, f.w, g.w, mk));
        }
    }
}

__global__ __launch_bounds__(256) void gate_bwd_reduce_row_kernel(const float* __restrict__ dy, const float* __restrict__ yf,
                                                                  const float* __restrict__ yg, int rows, int C, int S,
                                                                  GateBN bn, const float* __restrict__ mask,
                                                                  float* __restrict__ red) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const int c = row % C;
        const GateCh k = gate_ch(bn, c);
        const float mk = mask ? mask[row] : 1.0f;
        const size_t base = (size_t)row * S;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;      // dgamma_f, dbeta_f, dgamma_g, dbeta_g
        for (int s = lane * 4; s < S; s += 256) {
            const float4 f4 = ld4(yf + base + s), g4 = ld4(yg + base + s), d4 = ld4(dy + base + s);
            const float ff[4] = {f4.x, f4.y, f4.z, f4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) gate_red_add(v0, v1, v2, v3, k, gate_dz(k, ff[e], gg[e], dd[e], mk), ff[e], gg[e]);
        }
        v0 = wave_sum(v0); v1 = wave_sum(v1); v2 = wave_sum(v2); v3 = wave_sum(v3);
        if (lane == 0) {
            atomicAdd(red + c, v0);
            atomicAdd(red + C + c, v1);
            atomicAdd(red + 2 * C + c, v2);
            atomicAdd(red + 3 * C + c, v3);
        }
    }
}

__global__ __launch_bounds__(256) void gate_bwd_apply_row_kernel(const float* __restrict__ dy, const float* __restrict__ yf,
                                                                 const float* __restrict__ yg, int rows, int C, int S,
                                                                 GateBN bn, const float* __restrict__ mask,
                                                                 const float* __restrict__ red, float inv_count, int train,
                                                                 float* __restrict__ dyf, float* __restrict__ dyg) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const int c = row % C;
        const GateCh k = gate_ch(bn, c);
        const GateMeans m = gate_means(red, C, c, inv_count, train);
        const float mk = mask ? mask[row] : 1.0f;
        const size_t base = (size_t)row * S;
        for (int s = lane * 4; s < S; s += 256) {
            const float4 f4 = ld4(yf + base + s), g4 = ld4(yg + base + s), d4 = ld4(dy + base + s);
            const float ff[4] = {f4.x, f4.y, f4.z, f4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
            GatePair o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = gate_dx(k, gate_dz(k, ff[e], gg[e], dd[e], mk), {bn_xhat(ff[e], k.muf, k.isf), bn_xhat(gg[e], k.mug, k.isg)}, m);
            *reinterpret_cast<float4*>(dyf + base + s) = make_float4(o[0].f, o[1].f, o[2].f, o[3].f);
            *reinterpret_cast<float4*>(dyg + base + s) = make_float4(o[0].g, o[1].g, o[2].g, o[3].g);
        }
    }
}

// ---- one-pass backward forms (training mode, S % 4 == 0, a channel's N*S values fit the workgroup's registers):
// ONE workgroup of CH_THREADS (512) threads owns a whole channel.  It reads dy and the saved tensors once, keeps dz and the
// normalised input in registers across the block-wide reduction, then writes the input gradient: the two-pass forms
// above read every operand twice (and evaluate tanh / exp twice) -- 150 + 25 MB against 75 + 25 MB for a TCN
// BatchNorm at B = 32, 150 + 50 against 75 + 50 for the gate.  dgamma / dbeta are ADDED to red (one writer per
// channel, so no atomics), which lets the caller hand in the flat-gradient slots whether or not they are still zero.
constexpr int CH_THREADS = 512;
// register groups of four values per thread in the largest instantiation: with them, the largest N*S a channel may have
constexpr int BN_CH_MAX_PER = 16, GATE_CH_MAX_PER = 8;
static_assert(SELD_BN_ONE_PASS_MAX == CH_THREADS * BN_CH_MAX_PER * 4, "seld_hip.h states the BatchNorm one-pass limit");
static_assert(SELD_GATE_ONE_PASS_MAX == CH_THREADS * GATE_CH_MAX_PER * 4, "seld_hip.h states the gate one-pass limit");

template <int NV>
__device__ __forceinline__ void channel_block_sum(float (&v)[NV]) {
    __shared__ float part[NV][CH_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float s = wave_sum(v[k]);
        if (lane == 0) part[k][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < CH_THREADS / 64; ++w) t += part[k][w];
        v[k] = t;
    }
}

// group g of channel c (four values along S, G = N * S / 4 groups per channel): its batch item and float offset
struct ChannelPos { int n; size_t off; };
__device__ __forceinline__ ChannelPos channel_pos(int g, int c, int C, int S) {
    const int S4 = S >> 2, n = g / S4, s4 = g - n * S4;
    return {n, ((size_t)n * C + c) * S + (size_t)s4 * 4};
}

template <int PER>
__global__ __launch_bounds__(CH_THREADS) void bn_act_bwd_channel_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y, int N, int C, int S,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, int act,
    float* __restrict__ red, const float* __restrict__ dy2, float* __restrict__ dx, float inv_count) {
    const int c = blockIdx.x;
    const int G = N * (S >> 2);
    const float mu = mean[c], is = invstd[c], a = gamma[c] * is;
    float4 dz[PER], xh[PER];
    float v[2] = {0.f, 0.f};      // dgamma, dbeta
    // all loads first, from clamped addresses (see gate_bwd_channel_kernel)
    float4 ds_[PER], xs_[PER], ys_[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const size_t o = channel_pos(min((int)threadIdx.x + k * CH_THREADS, G - 1), c, C, S).off;
        ds_[k] = ld4(dy + o); xs_[k] = ld4(x + o); ys_[k] = ld4(y + o);
        if (dy2) {                           // y had two consumers: their gradients are summed here, not by a separate kernel
            const float4 e = ld4(dy2 + o);
            ds_[k].x += e.x; ds_[k].y += e.y; ds_[k].z += e.z; ds_[k].w += e.w;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int g = (int)threadIdx.x + k * CH_THREADS;
        dz[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        xh[k] = dz[k];
        if (g < G) {
            const float4 d = ds_[k];
            const float4 xx = xs_[k], yy = ys_[k];
            dz[k] = make_float4(bn_dz(d.x, yy.x, act), bn_dz(d.y, yy.y, act), bn_dz(d.z, yy.z, act), bn_dz(d.w, yy.w, act));
            xh[k] = make_float4(bn_xhat(xx.x, mu, is), bn_xhat(xx.y, mu, is), bn_xhat(xx.z, mu, is), bn_xhat(xx.w, mu, is));
            v[0] += dz[k].x * xh[k].x + dz[k].y * xh[k].y + dz[k].z * xh[k].z + dz[k].w * xh[k].w;
            v[1] += (dz[k].x + dz[k].y) + (dz[k].z + dz[k].w);
        }
    }
    channel_block_sum<2>(v);
    if (threadIdx.x == 0) {
        red[c] += v[0];
        red[C + c] += v[1];
    }
    if (!dx) return;
    const float k1 = v[1] * inv_count, k2 = v[0] * inv_count;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int g = (int)threadIdx.x + k * CH_THREADS;
        if (g < G) {
            const size_t o = channel_pos(g, c, C, S).off;
            float4 r = make_float4(bn_dx(a, dz[k].x, xh[k].x, k1, k2), bn_dx(a, dz[k].y, xh[k].y, k1, k2),
                                   bn_dx(a, dz[k].z, xh[k].z, k1, k2), bn_dx(a, dz[k].w, xh[k].w, k1, k2));
            *reinterpret_cast<float4*>(dx + o) = r;
        }
    }
}

template <int PER>
__global__ __launch_bounds__(CH_THREADS) void gate_bwd_channel_kernel(
    const float* __restrict__ dy, const float* __restrict__ yf, const float* __restrict__ yg, int N, int C, int S,
    GateBN bn, const float* __restrict__ mask, float* __restrict__ red, float* __restrict__ dyf,
    float* __restrict__ dyg, float inv_count) {
    const int c = blockIdx.x;
    const int G = N * (S >> 2);
    const GateCh ch = gate_ch(bn, c);
    float dzf[PER][4], dzg[PER][4], fh[PER][4], gh[PER][4];
    float v[4] = {0.f, 0.f, 0.f, 0.f};      // dgamma_f, dbeta_f, dgamma_g, dbeta_g
    // every operand of the channel is requested before the first one is used (unconditional loads from clamped addresses:
    // with the loads inside `if (g < G)` the compiler kept each group's load -> wait -> tanh / exp sequence in order, eight
    // exposed memory latencies per workgroup)
    float4 d4s[PER], f4s[PER], g4s[PER];
    float mks[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const ChannelPos p = channel_pos(min((int)threadIdx.x + k * CH_THREADS, G - 1), c, C, S);
        d4s[k] = ld4(dy + p.off); f4s[k] = ld4(yf + p.off); g4s[k] = ld4(yg + p.off);
        mks[k] = mask ? mask[p.n * C + c] : 1.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int g = (int)threadIdx.x + k * CH_THREADS;
#pragma unroll
        for (int e = 0; e < 4; ++e) dzf[k][e] = dzg[k][e] = fh[k][e] = gh[k][e] = 0.f;
        if (g < G) {
            const float4 d4 = d4s[k], f4 = f4s[k], g4 = g4s[k];
            const float mk = mks[k];
            const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, ff[4] = {f4.x, f4.y, f4.z, f4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const GatePair dz = gate_dz(ch, ff[e], gg[e], dd[e], mk);
                dzf[k][e] = dz.f;
                dzg[k][e] = dz.g;
                fh[k][e] = bn_xhat(ff[e], ch.muf, ch.isf);
                gh[k][e] = bn_xhat(gg[e], ch.mug, ch.isg);
                v[0] += dzf[k][e] * fh[k][e];
                v[1] += dzf[k][e];
                v[2] += dzg[k][e] * gh[k][e];
                v[3] += dzg[k][e];
            }
        }
    }
    channel_block_sum<4>(v);
    if (threadIdx.x == 0) {
        red[c] += v[0];
        red[C + c] += v[1];
        red[2 * C + c] += v[2];
        red[3 * C + c] += v[3];
    }
    GateMeans m;
    m.kf2 = v[0] * inv_count; m.kf1 = v[1] * inv_count; m.kg2 = v[2] * inv_count; m.kg1 = v[3] * inv_count;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int g = (int)threadIdx.x + k * CH_THREADS;
        if (g < G) {
            const size_t o = channel_pos(g, c, C, S).off;
            GatePair r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = gate_dx(ch, {dzf[k][e], dzg[k][e]}, {fh[k][e], gh[k][e]}, m);
            *reinterpret_cast<float4*>(dyf + o) = make_float4(r[0].f, r[1].f, r[2].f, r[3].f);
            *reinterpret_cast<float4*>(dyg + o) = make_float4(r[0].g, r[1].g, r[2].g, r[3].g);
        }
    }
}

}  // namespace seld

using namespace seld;
// chunks of a per-channel reduction: one (the block's single atomic add per output is then the only contribution) when
// SELD_DETERMINISTIC is set
static inline unsigned red_chunks(long long M) { return env().deterministic ? 1u : (unsigned)((M + RED_CHUNK - 1) / RED_CHUNK); }
// register groups per thread of the one-pass channel kernels: the smallest instantiation (1, 2, 4, ... max_per) whose
// CH_THREADS * PER groups of four hold the channel's N * S values, 0 when none does or S is not a multiple of 4
static inline int channel_groups(long long N, int S, int max_per) {
    if (S & 3) return 0;
    const long long G = N * S / 4;
    for (int p = 1; p <= max_per; p *= 2)
        if (G <= (long long)p * CH_THREADS) return p;
    return 0;
}
// f(std::integral_constant<int, PER>) for the instantiation `per` (a result of channel_groups(.., MAX_PER))
template <int MAX_PER, int P = 1, typename F>
static inline void with_channel_groups(int per, F&& f) {
    if constexpr (P < MAX_PER) {
        if (per != P) return with_channel_groups<MAX_PER, P * 2>(per, f);
    }
    f(std::integral_constant<int, P>{});
}
// the gate's one-wave-per-row forms
static inline bool gate_rows(long long N, long long C, int S) { return S % 4 == 0 && N * C < (1LL << 31); }
static inline bool gate_reduce_rows(long long N, long long C, int S) { return gate_rows(N, C, S) && !env().deterministic; }

extern "C" int seld_channel_stats(const float* x, int32_t N, int32_t C, int32_t S, float* stats, void* stream) {
    if (!x || !stats || N <= 0 || C <= 0 || S <= 0) return SELD_EINVAL;
    const long long M = (long long)N * S;
    dim3 grid(red_chunks(M), C);
    hipLaunchKernelGGL(channel_stats_kernel, grid, dim3(256), 0, ST(stream), x, N, C, S, stats);
    return check_launch();
}

extern "C" int seld_bn_finalize_ex(float* stats, int32_t C, int64_t count, float eps, float momentum, float* mean,
                                   float* invstd, float* running_mean, float* running_var,
                                   int64_t* num_batches_tracked, int32_t clear_stats, void* stream) {
    if (!stats || !mean || !invstd || C <= 0 || count <= 0) return SELD_EINVAL;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, ST(stream), stats, C, (double)count, eps,
                       momentum, mean, invstd, running_mean, running_var, (long long*)num_batches_tracked, clear_stats);
    return check_launch();
}

extern "C" int seld_bn_finalize2_ex(float* statsA, float* statsB, int32_t C, int64_t count, float eps, float momentum,
                                    float* meanA, float* invstdA, float* running_meanA, float* running_varA,
                                    int64_t* nbtA, float* meanB, float* invstdB, float* running_meanB,
                                    float* running_varB, int64_t* nbtB, int32_t clear_stats, void* stream) {
    if (!statsA || !statsB || !meanA || !invstdA || !meanB || !invstdB || C <= 0 || count <= 0) return SELD_EINVAL;
    const BnFin a{statsA, meanA, invstdA, running_meanA, running_varA, (long long*)nbtA};
    const BnFin b{statsB, meanB, invstdB, running_meanB, running_varB, (long long*)nbtB};
    hipLaunchKernelGGL(bn_finalize2_kernel, dim3((C + 3) / 4, 2), dim3(256), 0, ST(stream), a, b, C, (double)count, eps,
                       momentum, clear_stats);
    return check_launch();
}

extern "C" int seld_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps,
                                  float* mean, float* invstd, void* stream) {
    if (!running_mean || !running_var || !mean || !invstd || C <= 0) return SELD_EINVAL;
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, ST(stream), running_mean, running_var,
                       C, eps, mean, invstd);
    return check_launch();
}

extern "C" int seld_bn_act_fwd(const float* x, int32_t N, int32_t C, int32_t S, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, int32_t act, float* y, void* stream) {
    if (!x || !y || !mean || !invstd || !gamma || !beta) return SELD_EINVAL;
    const long long total = (long long)N * C * S;
    hipLaunchKernelGGL(bn_act_fwd_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, ST(stream), x, total, C, S, mean,
                       invstd, gamma, beta, act, y);
    return check_launch();
}

extern "C" int seld_bn_act_bwd_reduce(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                                      const float* mean, const float* invstd, const float* gamma, const float* beta,
                                      int32_t act, float* red, void* stream) {
    (void)gamma; (void)beta;
    if (!dy || !x || !y || !red) return SELD_EINVAL;
    const long long M = (long long)N * S;
    dim3 grid(red_chunks(M), C);
    hipLaunchKernelGGL(bn_act_bwd_reduce_kernel, grid, dim3(256), 0, ST(stream), dy, x, y, N, C, S, mean, invstd, act, red);
    return check_launch();
}

extern "C" int seld_bn_act_bwd_apply(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                                     const float* mean, const float* invstd, const float* gamma, const float* beta,
                                     int32_t act, const float* red, int32_t train, float* dx, void* stream) {
    (void)beta;
    if (!dy || !x || !y || !dx || (train && !red)) return SELD_EINVAL;
    const long long total = (long long)N * C * S;
    const float inv_count = 1.0f / (float)((long long)N * S);
    hipLaunchKernelGGL(bn_act_bwd_apply_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, ST(stream), dy, x, y, total,
                       C, S, mean, invstd, gamma, act, red, inv_count, train, dx);
    return check_launch();
}

// One-pass training-mode backward (see bn_act_bwd_channel_kernel).  SELD_EUNSUPPORTED when the channel does not fit
// the workgroup's registers or S is not a multiple of 4: the caller then takes the reduce + apply pair.
extern "C" int seld_bn_act_bwd_fused(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                                     const float* mean, const float* invstd, const float* gamma, int32_t act,
                                     float* red, const float* dy2, float* dx, void* stream) {
    if (!dy || !x || !y || !red || !mean || !invstd || !gamma || N <= 0 || C <= 0 || S <= 0) return SELD_EINVAL;
    const int per = channel_groups(N, S, BN_CH_MAX_PER);
    if (!per) return SELD_EUNSUPPORTED;
    const float inv_count = 1.0f / (float)((long long)N * S);
    with_channel_groups<BN_CH_MAX_PER>(per, [&](auto P) {
        hipLaunchKernelGGL(bn_act_bwd_channel_kernel<decltype(P)::value>, dim3(C), dim3(CH_THREADS), 0, ST(stream), dy, x, y, N,
                           C, S, mean, invstd, gamma, act, red, dy2, dx, inv_count);
    });
    return check_launch();
}

extern "C" int seld_gate_fwd(const float* yf, const float* yg, int32_t N, int32_t C, int32_t S, const float* mean_f,
                             const float* invstd_f, const float* gamma_f, const float* beta_f, const float* mean_g,
                             const float* invstd_g, const float* gamma_g, const float* beta_g, const float* mask,
                             float* y, void* stream) {
    if (!yf || !yg || !y) return SELD_EINVAL;
    const long long total = (long long)N * C * S;
    const GateBN bn{mean_f, invstd_f, gamma_f, beta_f, mean_g, invstd_g, gamma_g, beta_g};
    if (gate_rows(N, C, S))
        hipLaunchKernelGGL(gate_fwd_row_kernel, dim3(row_grid((long long)N * C)), dim3(256), 0, ST(stream), yf, yg, N * C, C, S,
                           bn, mask, y);
    else
        hipLaunchKernelGGL(gate_fwd_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, ST(stream), yf, yg, total, C, S,
                           bn, mask, y);
    return check_launch();
}

extern "C" int seld_gate_bwd_reduce(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                                    const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                                    const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                                    const float* mask, float* red, void* stream) {
    if (!dy || !yf || !yg || !red) return SELD_EINVAL;
    const long long M = (long long)N * S;
    dim3 grid(red_chunks(M), C);
    const GateBN bn{mean_f, invstd_f, gamma_f, beta_f, mean_g, invstd_g, gamma_g, beta_g};
    if (gate_reduce_rows(N, C, S))
        hipLaunchKernelGGL(gate_bwd_reduce_row_kernel, dim3(row_grid((long long)N * C)), dim3(256), 0, ST(stream), dy, yf, yg,
                           N * C, C, S, bn, mask, red);
    else
        hipLaunchKernelGGL(gate_bwd_reduce_kernel, grid, dim3(256), 0, ST(stream), dy, yf, yg, N, C, S, bn, mask, red);
    return check_launch();
}

extern "C" int seld_gate_bwd_apply(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                                   const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                                   const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                                   const float* mask, const float* red, int32_t train, float* dyf, float* dyg,
                                   void* stream) {
    if (!dy || !yf || !yg || !dyf || !dyg || (train && !red)) return SELD_EINVAL;
    const long long total = (long long)N * C * S;
    const float inv_count = 1.0f / (float)((long long)N * S);
    const GateBN bn{mean_f, invstd_f, gamma_f, beta_f, mean_g, invstd_g, gamma_g, beta_g};
    if (gate_rows(N, C, S))
        hipLaunchKernelGGL(gate_bwd_apply_row_kernel, dim3(row_grid((long long)N * C)), dim3(256), 0, ST(stream), dy, yf, yg,
                           N * C, C, S, bn, mask, red, inv_count, train, dyf, dyg);
    else
        hipLaunchKernelGGL(gate_bwd_apply_kernel, dim3(grid_for(total / 4 + 1)), dim3(256), 0, ST(stream), dy, yf, yg, total,
                           C, S, bn, mask, red, inv_count, train, dyf, dyg);
    return check_launch();
}

extern "C" int seld_gate_bwd_fused(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                                   const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                                   const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                                   const float* mask, float* red, float* dyf, float* dyg, void* stream) {
    if (!dy || !yf || !yg || !red || !dyf || !dyg || N <= 0 || C <= 0 || S <= 0) return SELD_EINVAL;
    const int per = channel_groups(N, S, GATE_CH_MAX_PER);
    if (!per) return SELD_EUNSUPPORTED;
    const float inv_count = 1.0f / (float)((long long)N * S);
    const GateBN bn{mean_f, invstd_f, gamma_f, beta_f, mean_g, invstd_g, gamma_g, beta_g};
    with_channel_groups<GATE_CH_MAX_PER>(per, [&](auto P) {
        hipLaunchKernelGGL(gate_bwd_channel_kernel<decltype(P)::value>, dim3(C), dim3(CH_THREADS), 0, ST(stream), dy, yf, yg, N,
                           C, S, bn, mask, red, dyf, dyg, inv_count);
    });
    return check_launch();
}

// Which kernel a BatchNorm / gate entry point launches for (N, C, S) under the current switches, from the same selection
// functions the entry points use.
extern "C" int seld_norm_kernel_label(int32_t op, int32_t N, int32_t C, int32_t S, char* buf, int32_t buflen) {
    if (N <= 0 || C <= 0 || S <= 0 || !buf || buflen < 48) return SELD_EINVAL;
    const long long M = (long long)N * S;
    const int vec = (S & 3) ? 1 : 4;
    switch (op) {
        case SELD_NORM_BN_BWD_FUSED:
        case SELD_NORM_GATE_BWD_FUSED: {
            const bool bn = op == SELD_NORM_BN_BWD_FUSED;
            const int per = channel_groups(N, S, bn ? BN_CH_MAX_PER : GATE_CH_MAX_PER);
            if (!per) return SELD_EUNSUPPORTED;
            snprintf(buf, buflen, "%s_bwd_channel_kernel<%d>", bn ? "bn_act" : "gate", per);
            return SELD_OK;
        }
        case SELD_NORM_BN_BWD_REDUCE:
            snprintf(buf, buflen, "bn_act_bwd_reduce_kernel[x%d, %u chunks]", vec, red_chunks(M));
            return SELD_OK;
        case SELD_NORM_BN_BWD_APPLY:
            snprintf(buf, buflen, "bn_act_bwd_apply_kernel[x%d]", vec);
            return SELD_OK;
        case SELD_NORM_GATE_FWD:
            snprintf(buf, buflen, gate_rows(N, C, S) ? "gate_fwd_row_kernel" : "gate_fwd_kernel");
            return SELD_OK;
        case SELD_NORM_GATE_BWD_REDUCE:
            if (gate_reduce_rows(N, C, S)) snprintf(buf, buflen, "gate_bwd_reduce_row_kernel");
            else snprintf(buf, buflen, "gate_bwd_reduce_kernel[x%d, %u chunks]", vec, red_chunks(M));
            return SELD_OK;
        case SELD_NORM_GATE_BWD_APPLY:
            snprintf(buf, buflen, gate_rows(N, C, S) ? "gate_bwd_apply_row_kernel" : "gate_bwd_apply_kernel");
            return SELD_OK;
        default:
            return SELD_EINVAL;
    }
}
